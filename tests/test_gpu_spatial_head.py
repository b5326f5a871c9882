"""Float64 parity of the streaming kernels around the convolutions (-m gpu): max-pool 2x2, bilinear x2, zero fill
(spatial.hip) and the 1x1 head (head_adam.hip), on every launch path of their extern "C" dispatchers and on the layouts the
engine hands them.  References and layouts: tests/spatial_cases.py (validated on the host by
test_spatial_reference_host.py).  Every tensor a kernel writes lives in a sentinel-filled allocation; after the call
everything outside the written planes must still hold the sentinel.

Layouts (spatial_cases.Layout): dense; lo / hi = channels [0, C) / [C, 2C) of a contiguous 2C-channel buffer (batch
stride 2 C H W: the [up | skip] concat buffers, the fused two-lane buffers); padN = batch stride C H W + N.  The padded
strides exist to reach the fall-backs keyed on the batch stride; which kernel a case is meant to reach is derived from
the dispatch conditions and stated in its `target` (part of the test id) and in the comment of its table.

Tolerances, of max |reference|: bilinear 5e-6 forward and 1e-5 backward (test_upsample_bilinear's), head 2e-5 (_close of
test_gpu_kernels.py); pooling and fill are exact."""
import pytest
import torch

import spatial_cases as S
from spatial_cases import Layout as L

pytestmark = pytest.mark.gpu

UP_FWD_TOL, UP_BWD_TOL, HEAD_TOL = 5e-6, 1e-5, 2e-5


def _bf16_allow(got, ref, bf16_out):
    """test_bf16_stored_activations' allowance for the bilinear instantiations: an fp32 ulp (separate instantiations may
    contract the interpolation FMAs differently), a bf16 ulp where the result is narrowed"""
    err = (got.float() - ref.float()).abs()
    return float((err - (2.0 ** -8 if bf16_out else 1e-6) * ref.float().abs()).max()) <= 1e-6


# ================================================================================================ max-pool
# aide_maxpool2x2_fwd takes maxpool2x2_fwd_scalar_kernel when W % 4 || x_bs % 4 || y_bs % 2, else
# maxpool2x2_fwd_kernel<float, float>; aide_maxpool2x2_bwd takes maxpool2x2_bwd_scalar_kernel when
# W % 4 || x_bs % 4 || dx_bs % 4 || dy_bs % 2, else maxpool2x2_bwd_kernel<float, float, float>.
#   W in {4, 8, 24}: C H W % 4 == 0 and C (H/2) (W/2) % 2 == 0, so
#       dense, slice (x / dx = hi half, y / dy = lo half), pad4   -> the vector kernels (strides 1x, 2x, +4)
#       pad1 (every stride odd), pad2 (x_bs % 4 == 2)             -> the scalar kernels at W % 4 == 0
#   W in {2, 6, 10, 18}: W % 4 != 0                               -> the scalar kernels on every layout
POOL_W_VEC, POOL_W_SCALAR, POOL_H = (4, 8, 24), (2, 6, 10, 18), (2, 6, 16)
POOL_KINDS = {'dense': ('dense', 'dense'), 'slice': ('hi', 'lo'), 'pad1': ('pad1', 'pad1'), 'pad2': ('pad2', 'pad2'),
              'pad4': ('pad4', 'pad4')}            # (layout of x and dx, layout of y and dy)


def _pool_target(w, kind):
    vec = w % 4 == 0 and kind in ('dense', 'slice', 'pad4')
    return 'maxpool2x2_fwd_kernel+maxpool2x2_bwd_kernel' if vec else 'maxpool2x2_fwd_scalar_kernel+maxpool2x2_bwd_scalar_kernel'


def _pool_check(dev, case, kx, ky, kdx=None, what=''):
    from aide_amd import ops
    x, dy, base, y_ref, dx_ref = case
    kdx = kdx or kx
    _, xv = L(kx, x.shape).put(x, dev)
    ly = L(ky, y_ref.shape)
    fy, yv = ly.blank(dev)
    ops.maxpool2x2_fwd(xv, yv)
    assert torch.equal(yv.cpu(), y_ref), 'forward ' + what
    assert ly.intact(fy), 'forward wrote outside its planes ' + what
    _, gv = ly.put(dy, dev)
    ld = L(kdx, x.shape)
    fd, dv = ld.blank(dev)
    ops.maxpool2x2_bwd(xv, gv, dv, accumulate=False)
    assert torch.equal(dv.cpu(), dx_ref), 'backward ' + what
    assert ld.intact(fd), 'backward wrote outside its planes ' + what
    fd, dv = ld.put(base, dev)                     # accumulate onto a non-constant base: one fp32 add per element, exact
    ops.maxpool2x2_bwd(xv, gv, dv, accumulate=True)
    assert torch.equal(dv.cpu(), base + dx_ref), 'accumulating backward ' + what
    assert ld.intact(fd), 'accumulating backward wrote outside its planes ' + what


@pytest.mark.parametrize('kind', sorted(POOL_KINDS))
@pytest.mark.parametrize('w', POOL_W_VEC + POOL_W_SCALAR)
def test_pool(dev, w, kind):
    """forward, backward, accumulating backward == aten bit for bit on tie content (whole windows equal, ties across the
    window rows, negative-only, -inf planes, +0.0 against -0.0); target kernels: _pool_target(w, kind)"""
    kx, ky = POOL_KINDS[kind]
    for h in POOL_H:
        _pool_check(dev, S.pool_case(2, 5, h, w), kx, ky, what='%dx%d %s -> %s' % (h, w, kind, _pool_target(w, kind)))


# one operand alone on an odd / 2 mod 4 stride, W = 8: each term of the two dispatch conditions on its own
#   x pad2 (x_bs % 4), y / dy pad1 (y_bs % 2, dy_bs % 2), dx pad2 (dx_bs % 4)   -> the scalar kernels
@pytest.mark.parametrize('which', ['x', 'y', 'dx'])
def test_pool_one_operand_padded(dev, which):
    case = S.pool_case(2, 5, 6, 8)
    _pool_check(dev, case, 'pad2' if which == 'x' else 'dense', 'pad1' if which == 'y' else 'dense',
                'pad2' if which == 'dx' else 'dense', what='only %s padded -> scalar kernels' % which)


@pytest.mark.parametrize('w', [8, 6])          # maxpool2x2_*_kernel / maxpool2x2_*_scalar_kernel
def test_pool_two_launch_split(dev, w):
    """the engine pools [0, c) and [c, C) of a fused buffer on two lanes: two launches over channel slices of x, y, dy, dx
    == one launch over all channels, bit for bit"""
    from aide_amd import ops
    x, dy, base, y_ref, dx_ref = S.pool_case(2, 5, 6, w)
    xd, gd, c = x.to(dev), dy.to(dev), 2
    y1, y2 = torch.full_like(gd, S.SENT), torch.full_like(gd, S.SENT)
    ops.maxpool2x2_fwd(xd, y1)
    ops.maxpool2x2_fwd(xd[:, :c], y2[:, :c])
    assert torch.equal(y2[:, :c], y1[:, :c]) and bool((y2[:, c:] == S.SENT).all())
    ops.maxpool2x2_fwd(xd[:, c:], y2[:, c:])
    assert torch.equal(y2, y1) and torch.equal(y1.cpu(), y_ref)
    for acc in (False, True):
        d1, d2 = base.to(dev), base.to(dev)
        ops.maxpool2x2_bwd(xd, gd, d1, accumulate=acc)
        ops.maxpool2x2_bwd(xd[:, :c], gd[:, :c], d2[:, :c], accumulate=acc)
        assert torch.equal(d2[:, c:].cpu(), base[:, c:])
        ops.maxpool2x2_bwd(xd[:, c:], gd[:, c:], d2[:, c:], accumulate=acc)
        assert torch.equal(d2, d1) and torch.equal(d1.cpu(), base + dx_ref if acc else dx_ref)


# more threads than the 8192 x 256 grid cap, so the grid-stride loops run a second iteration:
#   8 x 64 x 256 x 256: 4 194 304 threads of maxpool2x2_fwd_kernel / maxpool2x2_bwd_kernel (vector: W % 4 == 0, dense)
#   8 x 64 x 130 x 130: 2 163 200 threads of the two scalar kernels (W % 4 == 2)
# measured on MI355X: both bit-equal to aten (max error 0)
@pytest.mark.parametrize('shape', [(8, 64, 256, 256), (8, 64, 130, 130)])
def test_pool_beyond_the_grid_cap(dev, shape):
    from aide_amd import ops
    n, c, h, w = shape
    assert n * c * (h // 2) * (w // (4 if w % 4 == 0 else 2)) > 8192 * 256
    g = torch.Generator().manual_seed(h)
    x = torch.randint(-8, 9, shape, generator=g).float() * 0.25            # ties in about a fifth of the windows
    dy = torch.randn(n, c, h // 2, w // 2, generator=g)
    y_ref, dx_ref = S.pool_ref(x, dy)
    xd = x.to(dev)
    y = torch.full(y_ref.shape, S.SENT, device=dev)
    ops.maxpool2x2_fwd(xd, y)
    assert torch.equal(y.cpu(), y_ref)
    dx = torch.full(shape, S.SENT, device=dev)
    ops.maxpool2x2_bwd(xd, dy.to(dev), dx)
    assert torch.equal(dx.cpu(), dx_ref)


# ================================================================================================ bilinear x2, forward
# aide_upsample2x_bilinear_fwd: (2W) % 4 == 0 && y_bs % 4 == 0 -> upsample_fwd_t, which takes
# upsample2x_fwd_tiled_kernel<float, float> when (2H) % 32 == 0 && (2W) % 128 == 0 && x_bs % 4 == 0 && y_bs % 8 == 0, else
# upsample2x_fwd_vec_kernel<float, float>; everything else -> upsample2x_fwd_kernel (scalar).  The destination's
# C 2H 2W is a multiple of 4 (of 8 on the tiled shapes), so its padding alone decides y_bs % 4 / % 8.
# (The vector kernel clamps its four source columns to W - 1 only to keep the loads inside the row: w1 <= W - 1, so no
# output selects a clamped column and their values cannot show; a clamp that is wrong by one, W - 2, fails every shape here.)
UP_ODD_W, UP_ODD_H = (1, 3, 5, 7, 511), (1, 3, 7)
UP_VEC = ((8, 8), (20, 12), (6, 10), (3, 510))
UP_TILED = ((16, 64), (48, 192), (16, 512))
UP_FWD = []         # (h, w, layout of x, layout of y, target)
for _hw in UP_VEC:
    UP_FWD += [_hw + ('dense', 'dense', 'upsample2x_fwd_vec_kernel'),
               _hw + ('hi', 'lo', 'upsample2x_fwd_vec_kernel'),          # into the `up` half of [up | skip]: y_bs = 2 C 2H 2W
               _hw + ('pad1', 'pad4', 'upsample2x_fwd_vec_kernel'),      # y_bs % 4 == 0 still; the source is read by element
               _hw + ('dense', 'pad1', 'upsample2x_fwd_kernel'),         # even W, y_bs odd: the scalar kernel
               _hw + ('dense', 'pad2', 'upsample2x_fwd_kernel')]         # even W, y_bs % 4 == 2: the scalar kernel
for _hw in UP_TILED:
    UP_FWD += [_hw + ('dense', 'dense', 'upsample2x_fwd_tiled_kernel'),
               _hw + ('hi', 'lo', 'upsample2x_fwd_tiled_kernel'),        # both strides doubled: still whole aligned tiles
               _hw + ('dense', 'pad4', 'upsample2x_fwd_vec_kernel'),     # y_bs % 8 == 4: the vector instead of the tiled kernel
               _hw + ('pad2', 'dense', 'upsample2x_fwd_vec_kernel'),     # x_bs % 4 == 2: no aligned source window, vector
               _hw + ('dense', 'pad2', 'upsample2x_fwd_kernel')]


def _up_fwd_check(dev, h, w, kx, ky, what):
    from aide_amd import ops
    x, _, _, y_ref, _ = S.up_case(2, 3, h, w)
    _, xv = L(kx, x.shape).put(x, dev)
    ly = L(ky, y_ref.shape)
    fy, yv = ly.blank(dev)
    ops.upsample2x_fwd(xv, yv)
    S.assert_close(yv, y_ref, UP_FWD_TOL, 'forward ' + what)
    assert ly.intact(fy), 'forward wrote outside its planes ' + what


@pytest.mark.parametrize('case', UP_FWD, ids=lambda c: '%dx%d-%s-%s-%s' % c)
def test_upsample_fwd(dev, case):
    h, w, kx, ky, target = case
    _up_fwd_check(dev, h, w, kx, ky, '%s' % (case,))


# odd W: (2W) % 4 == 2 -> upsample2x_fwd_kernel on every layout (1 x 1 .. 7 x 511: single rows / columns, where
# scale = 0 / 1, and the widest odd row)
@pytest.mark.parametrize('kinds', [('dense', 'dense'), ('hi', 'lo'), ('pad1', 'pad1'), ('pad4', 'pad2')], ids='-'.join)
@pytest.mark.parametrize('w', UP_ODD_W)
def test_upsample_fwd_odd_width(dev, w, kinds):
    for h in UP_ODD_H:
        _up_fwd_check(dev, h, w, kinds[0], kinds[1], '%dx%d %s -> upsample2x_fwd_kernel' % (h, w, kinds))


# ================================================================================================ bilinear x2, backward
# aide_upsample2x_bilinear_bwd: dy_bs odd -> upsample2x_bwd_kernel (gather); else the tiled kernel, FAST when the gradient's
# pointer and batch stride are 16-byte aligned and (2W) % 4 == 0, the plain loader otherwise.  The gradient's C 2H 2W is
# a multiple of 4, so:
#   dense / lo (the `up` half of a concat gradient), even W      -> upsample2x_bwd_tiled_kernel<float, float, true>
#   dense / lo, odd W ((2W) % 4 == 2); pad2 at any W             -> upsample2x_bwd_tiled_kernel<float, float, false>
#   pad1                                                         -> upsample2x_bwd_kernel
# dx is written by element in all of them: its layout (hi, pad1) only moves the addresses.
UP_RAGGED = ((20, 80), (18, 160), (33, 130))        # more than one 64-column tile, not whole tiles (and 33 rows: three row tiles)
UP_BWD_KINDS = {'dense': ('dense', 'dense'), 'slice': ('lo', 'hi'), 'gpad1': ('pad1', 'dense'), 'gpad2': ('pad2', 'dense'),
                'dxpad1': ('dense', 'pad1')}         # (layout of the gradient dy, layout of dx)


def _up_bwd_target(w, kind):
    if kind == 'gpad1':
        return 'upsample2x_bwd_kernel'
    return 'upsample2x_bwd_tiled_kernel<%s>' % ('FAST' if w % 2 == 0 and kind != 'gpad2' else 'plain')


def _up_bwd_check(dev, n, c, h, w, kind):
    from aide_amd import ops
    _, dy, base, _, dx_ref = S.up_case(n, c, h, w)
    kg, kd = UP_BWD_KINDS[kind]
    what = '%dx%dx%dx%d %s -> %s' % (n, c, h, w, kind, _up_bwd_target(w, kind))
    fg, gv = L(kg, dy.shape).put(dy, dev)
    ld = L(kd, base.shape)
    fd, dv = ld.blank(dev)
    ops.upsample2x_bwd(gv, dv, accumulate=False)
    S.assert_close(dv, dx_ref, UP_BWD_TOL, 'backward ' + what)
    assert ld.intact(fd), 'backward wrote outside its planes ' + what
    fd, dv = ld.put(base, dev)
    ops.upsample2x_bwd(gv, dv, accumulate=True)
    S.assert_close(dv, base.double() + dx_ref, UP_BWD_TOL, 'accumulating backward ' + what)
    assert ld.intact(fd), 'accumulating backward wrote outside its planes ' + what


@pytest.mark.parametrize('kind', sorted(UP_BWD_KINDS))
@pytest.mark.parametrize('hw', UP_VEC + UP_TILED + UP_RAGGED, ids=lambda s: '%dx%d' % s)
def test_upsample_bwd(dev, hw, kind):
    """overwrite and accumulate; target kernel: _up_bwd_target(w, kind).  (16, 512) and (3, 510) go past column 384, where the
    one-ulp index bugs recorded in spatial.hip lived (columns 191 and 335)"""
    _up_bwd_check(dev, 2, 3, hw[0], hw[1], kind)


@pytest.mark.parametrize('kind', sorted(UP_BWD_KINDS))
@pytest.mark.parametrize('w', UP_ODD_W)
def test_upsample_bwd_odd_width(dev, w, kind):
    """odd W: the plain loader of the tiled kernel (gather kernel on gpad1), 1 x 1 included"""
    for h in UP_ODD_H:
        _up_bwd_check(dev, 2, 3, h, w, kind)


@pytest.mark.parametrize('kind', ['dense', 'gpad2', 'gpad1'])
def test_upsample_bwd_plane_groups(dev, kind):
    """7 x 191 planes of 2 x 2: one tile position, ub_plane_groups = 1280 workgroups that walk planes g, g + 1280: 57 of them
    take a second plane, the others stop after one (tiled kernel, FAST / plain; the gather kernel for comparison)"""
    _up_bwd_check(dev, 7, 191, 2, 2, kind)


# ================================================================================================ head
# head_fwd_t / head_bwd_t instantiate head_fwd_kernel<K, XT>, head_dgrad_kernel<K, DT>, head_wgrad_kernel<K, XT> for
# K = 1 .. 8 (aide_pick) and finish with head_wgrad_finalize_kernel; fp32 storage reaches them through
# aide_head1x1_fwd_mixed / aide_head1x1_bwd_mixed with XT = DT = float.  The weight gradient walks channels -1 (bias),
# 0, 1, ... in groups of 8 (K <= 4) or 4 (K > 4): C = 2 does not fill the first group, 7 fills the K <= 4 group exactly
# (with the bias) and leaves a ragged one for K > 4, 16 and 64 leave one channel for a last group, 67 leaves four.
# Layouts: batch strides must be multiples of 4, so dense, hi / lo and pad4 run; pad1 / pad2 are refused.
HEAD_C = (2, 7, 16, 64, 67)
HEAD_KINDS = (('dense', 'dense'), ('hi', 'lo'), ('pad4', 'pad4'))       # (x and dx, logits and dlogits)


def _small(dev, n):
    """a guarded 1-D fp32 output (dw, db)"""
    flat = torch.full((n + 2 * S.GUARD,), S.SENT, device=dev)
    return flat, flat[S.GUARD:S.GUARD + n]


def _small_intact(flat, n):
    return bool((flat[:S.GUARD] == S.SENT).all()) and bool((flat[S.GUARD + n:] == S.SENT).all())


def _head_check(dev, d, kx, ky, ws=None, bn=False):
    """forward with / without bias, dgrad + wgrad + dbias, dw=None, dx=None on one layout pair; bn: the _bn entry points
    (forward, weight / bias gradient; their data gradient belongs to aide_bn_relu_bwd_head)"""
    from aide_amd import ops
    n, c, h, w = d['x'].shape
    k = d['w'].shape[0]
    what = 'K=%d C=%d %s/%s%s' % (k, c, kx, ky, ' bn' if bn else '')
    _, xv = L(kx, d['x'].shape).put(d['x'], dev)
    wd, bd = d['w'].to(dev), d['b'].to(dev)
    sc, sh = (d['scale'].to(dev), d['shift'].to(dev)) if bn else (None, None)
    ly = L(ky, d['y'].shape)
    for bias, ref in ((bd, d['y']), (None, d['y_nobias'])):
        fy, yv = ly.blank(dev)
        if bn:
            ops.head1x1_fwd_bn(xv, sc, sh, wd, bias, yv)
        else:
            ops.head1x1_fwd(xv, wd, bias, yv)
        S.assert_close(yv, ref, HEAD_TOL, 'logits (bias %s) %s' % (bias is not None, what))
        assert ly.intact(fy), 'forward wrote outside its planes ' + what
    _, gv = ly.put(d['dy'], dev)
    fw, dw = _small(dev, k * c)
    fb, db = _small(dev, k)
    if bn:
        ops.head1x1_wgrad_bn(gv, xv, sc, sh, dw.view(k, c), db, ws=ws)
    else:
        ld = L(kx, d['x'].shape)
        fd, dv = ld.blank(dev)
        ops.head1x1_bwd(gv, xv, wd, dv, dw.view(k, c), db, ws=ws)
        S.assert_close(dv, d['dx'], HEAD_TOL, 'dx ' + what)
        assert ld.intact(fd), 'dgrad wrote outside its planes ' + what
    S.assert_close(dw.view(k, c), d['dw'], HEAD_TOL, 'dw ' + what)
    S.assert_close(db, d['db'], HEAD_TOL, 'db ' + what)
    assert _small_intact(fw, k * c) and _small_intact(fb, k), 'wgrad wrote outside dw / db ' + what
    if bn:
        return
    fd, dv = ld.blank(dev)                                   # data gradient only
    ops.head1x1_bwd(gv, xv, wd, dv, None, None, ws=ws)
    S.assert_close(dv, d['dx'], HEAD_TOL, 'dx (dw=None) ' + what)
    assert ld.intact(fd)
    fw, dw = _small(dev, k * c)                              # weight / bias gradient only
    fb, db = _small(dev, k)
    ops.head1x1_bwd(gv, xv, wd, None, dw.view(k, c), db, ws=ws)
    S.assert_close(dw.view(k, c), d['dw'], HEAD_TOL, 'dw (dx=None) ' + what)
    S.assert_close(db, d['db'], HEAD_TOL, 'db (dx=None) ' + what)
    assert _small_intact(fw, k * c) and _small_intact(fb, k)


@pytest.mark.parametrize('c', HEAD_C)
@pytest.mark.parametrize('k', range(1, 9))
def test_head(dev, k, c):
    """head_fwd_kernel<K, float>, head_dgrad_kernel<K, float>, head_wgrad_kernel<K, float> + head_wgrad_finalize_kernel
    against float64 conv2d, 2 x C x 8 x 12"""
    d = S.head_case(2, c, k, 8, 12)
    for kx, ky in HEAD_KINDS:
        _head_check(dev, d, kx, ky)


@pytest.mark.parametrize('c', [7, 64])
@pytest.mark.parametrize('k', [2, 5, 8])
def test_head_bn(dev, k, c):
    """aide_head1x1_fwd_bn / aide_head1x1_wgrad_bn (head_fwd_kernel / head_wgrad_kernel with in_scale: BatchNorm + ReLU
    applied while z is read) against the float64 head on relu(z * scale + shift); about half of the activations clipped"""
    d = S.head_case(2, c, k, 8, 12, bn=True)
    for kx, ky in HEAD_KINDS:
        _head_check(dev, d, kx, ky, bn=True)


def test_head_shared_workspace(dev):
    """two different (C, K) back to back on one workspace, as the engine's head_ws serves every head of a plan: partial rows
    of the first call (stride K C + K) must not leak into the second; the workspace starts as garbage"""
    from aide_amd._lib import lib
    nbytes = max(lib.aide_head1x1_ws_bytes(64, 2), lib.aide_head1x1_ws_bytes(7, 5), lib.aide_head1x1_ws_bytes(67, 8))
    ws = torch.full((nbytes // 8,), 1e30, device=dev, dtype=torch.float64)
    for c, k in ((64, 2), (7, 5), (67, 8), (64, 2)):
        _head_check(dev, S.head_case(2, c, k, 8, 12), 'dense', 'dense', ws=ws)
    _head_check(dev, S.head_case(2, 7, 5, 8, 12, bn=True), 'dense', 'dense', ws=ws, bn=True)


# N H W / 4 = 327 680 pixel quads > 1024 x 256: every workgroup of head_wgrad_kernel<3, float> runs its stride loop twice
# (the forward and the data gradient stay inside their 4096 x 256 grids).
# measured on MI355X, of max |ref|: logits 1.38e-7, dx 6.02e-8, dw 3.68e-8, db 7.43e-8 (bound 2e-5)
def test_head_wgrad_stride_loop(dev):
    from aide_amd import ops
    n, c, k, h, w = 5, 8, 3, 512, 512
    assert n * h * w // 4 > 1024 * 256
    g = torch.Generator().manual_seed(12)
    x = torch.randn(n, c, h, w, generator=g)
    wt, b = torch.randn(k, c, generator=g) * 0.3, torch.randn(k, generator=g)
    dy = torch.randn(n, k, h, w, generator=g)
    y_ref, dx_ref, dw_ref, db_ref = S.head_ref(x, wt, b, dy)
    xd, wd, gd = x.to(dev), wt.to(dev), dy.to(dev)
    y = torch.full(dy.shape, S.SENT, device=dev)
    ops.head1x1_fwd(xd, wd, b.to(dev), y)
    S.assert_close(y, y_ref, HEAD_TOL, 'logits')
    dx = torch.full(x.shape, S.SENT, device=dev)
    dw, db = torch.full((k, c), S.SENT, device=dev), torch.full((k,), S.SENT, device=dev)
    ops.head1x1_bwd(gd, xd, wd, dx, dw, db)
    print('head stride loop: logits %.2e dx %.2e dw %.2e db %.2e' % (S.rel_err(y, y_ref), S.rel_err(dx, dx_ref),
                                                                    S.rel_err(dw, dw_ref), S.rel_err(db, db_ref)))
    S.assert_close(dx, dx_ref, HEAD_TOL, 'dx')
    S.assert_close(dw, dw_ref, HEAD_TOL, 'dw')
    S.assert_close(db, db_ref, HEAD_TOL, 'db')


def test_head_refuses(dev):
    """H W % 4 != 0, K = 0 and K = 9 (MAXK = 8), batch strides that are no multiple of 4: AIDE_ERR_ARG, nothing launched"""
    from aide_amd import ops

    def run(n, c, k, h, w, kx='dense', ky='dense', kout=None):
        x = torch.randn(n, c, h, w)
        _, xv = L(kx, x.shape).put(x, dev)
        wd, bd = torch.zeros(k, c, device=dev), torch.zeros(k, device=dev)
        ly = L(ky, (n, kout or k, h, w))
        fy, yv = ly.blank(dev)
        with pytest.raises(RuntimeError):
            ops.head1x1_fwd(xv, wd, bd, yv)
        with pytest.raises(RuntimeError):
            ops.head1x1_fwd_bn(xv, torch.ones(c, device=dev), torch.zeros(c, device=dev), wd, bd, yv)
        fd, dv = L(kx, x.shape).blank(dev)
        dw, db = torch.full((k, c), S.SENT, device=dev), torch.full((k,), S.SENT, device=dev)
        ws = torch.zeros(1024 * (10 * c + 10), device=dev, dtype=torch.float64)
        with pytest.raises(RuntimeError):
            ops.head1x1_bwd(yv, xv, wd, dv, dw, db, ws=ws)
        with pytest.raises(RuntimeError):
            ops.head1x1_wgrad_bn(yv, xv, torch.ones(c, device=dev), torch.zeros(c, device=dev), dw, db, ws=ws)
        torch.cuda.synchronize()
        assert bool((fy == S.SENT).all()) and bool((fd == S.SENT).all()) and bool((dw == S.SENT).all()) and bool((db == S.SENT).all())

    run(2, 4, 2, 3, 3)                       # H W = 9
    run(2, 4, 2, 2, 3)                       # H W = 6
    run(2, 4, 9, 4, 4)                       # K = 9
    run(2, 4, 0, 4, 4, kout=1)               # K = 0 (the logits tensor needs a channel to exist)
    run(2, 4, 2, 4, 4, kx='pad1')            # x_bs % 4 == 1
    run(2, 4, 2, 4, 4, kx='pad2')            # x_bs % 4 == 2
    run(2, 4, 2, 4, 4, ky='pad2')            # y_bs / dy_bs % 4 == 2


# ================================================================================================ zero fill
# aide_fill_zero: C H W % 4 || bs % 4 -> fill_zero_scalar_kernel, else fill_zero_kernel (16-byte stores).
FILL = [((2, 4, 6, 8), 'dense', 'fill_zero_kernel'), ((2, 4, 6, 8), 'hi', 'fill_zero_kernel'), ((2, 4, 6, 8), 'lo', 'fill_zero_kernel'),
        ((3, 4, 6, 8), 'pad4', 'fill_zero_kernel'),                     # bs % 4 == 0 with a gap
        ((3, 4, 6, 8), 'pad1', 'fill_zero_scalar_kernel'),              # bs odd
        ((3, 4, 6, 8), 'pad2', 'fill_zero_scalar_kernel'),              # bs % 4 == 2
        ((2, 3, 3, 5), 'dense', 'fill_zero_scalar_kernel'),             # C H W = 45
        ((2, 3, 3, 5), 'hi', 'fill_zero_scalar_kernel'), ((3, 3, 3, 5), 'pad1', 'fill_zero_scalar_kernel'),
        ((2, 1, 3, 6), 'lo', 'fill_zero_scalar_kernel'),                # C H W = 18: even, not a multiple of 4
        # 2 621 440 16-byte stores > 8192 x 256: the grid-stride loop of fill_zero_kernel runs twice
        ((4, 40, 256, 256), 'hi', 'fill_zero_kernel')]


@pytest.mark.parametrize('case', FILL, ids=lambda c: '%s-%s-%s' % ('x'.join(map(str, c[0])), c[1], c[2]))
def test_fill_zero(dev, case):
    from aide_amd import ops
    shape, kind, _ = case
    lay = L(kind, shape)
    flat, v = lay.blank(dev)
    ops.fill_zero(v)
    assert float(v.abs().max()) == 0.0 and not bool(torch.signbit(v).any())
    assert lay.intact(flat)


# ================================================================================================ bf16 storage
# The bf16 instantiations (precision='bf16'), held to test_bf16_stored_activations' contract on dense tensors and channel
# slices: bit-equal to the fp32-storage kernel on the widened input, narrowed RNE; the bilinear ones to that test's ulp
# allowance.  The fp32 side of each comparison is anchored to float64 by the tests above.
BF16_KINDS = (('dense', 'dense'), ('hi', 'lo'))
BF, FP = torch.bfloat16, torch.float32


@pytest.mark.parametrize('kinds', BF16_KINDS, ids='-'.join)
def test_bf16_pool(dev, kinds):
    """maxpool2x2_fwd_kernel<XT, YT> for the three mixed (XT, YT) and maxpool2x2_bwd_kernel<XT, GT, DT> for the seven mixed
    (XT, GT, DT), 2 x 16 x 8 x 24, overwrite and accumulate"""
    from aide_amd import ops
    kx, ky = kinds
    shape = (2, 16, 8, 24)
    x = S.pool_input(*shape, seed=5)
    x[0, 3] = -4.0                                                        # (-inf is covered in fp32; keep the widened sums finite)
    g = torch.Generator().manual_seed(77)
    dy = torch.randn(2, 16, 4, 12, generator=g).bfloat16().float()
    base = torch.randn(shape, generator=g).bfloat16().float()
    y_ref, dx_ref = S.pool_ref(x, dy)                                     # (half-integers: exact in bf16)
    lx, ly = L(kx, shape), L(ky, y_ref.shape)
    for xt in (BF, FP):
        _, xv = lx.put(x, dev, xt)
        for yt in (BF, FP):
            if (xt, yt) == (FP, FP):
                continue
            fy, yv = ly.blank(dev, yt)
            ops.maxpool2x2_fwd(xv, yv)
            assert torch.equal(yv.float().cpu(), y_ref) and ly.intact(fy), 'forward %s -> %s' % (xt, yt)
        for gt in (BF, FP):
            _, gv = ly.put(dy, dev, gt)
            for dt in (BF, FP):
                if (xt, gt, dt) == (FP, FP, FP):
                    continue
                for acc in (False, True):
                    fd, dv = lx.put(base, dev, dt)
                    ops.maxpool2x2_bwd(xv, gv, dv, accumulate=acc)
                    ref = (base + dx_ref) if acc else dx_ref
                    if dt == BF:
                        ref = ref.bfloat16().float()
                    assert torch.equal(dv.float().cpu(), ref) and lx.intact(fd), 'backward %s %s %s acc %s' % (xt, gt, dt, acc)


@pytest.mark.parametrize('kinds', BF16_KINDS, ids='-'.join)
@pytest.mark.parametrize('hw', [(8, 10), (8, 12), (20, 80), (16, 64)], ids=lambda s: '%dx%d' % s)
def test_bf16_upsample(dev, hw, kinds):
    """forward: upsample2x_fwd_vec_kernel<XT, YT> ((8, 10), (8, 12), (20, 80)) and upsample2x_fwd_tiled_kernel<XT, YT> ((16, 64))
    for the three mixed (XT, YT); backward: upsample2x_bwd_tiled_kernel<GT, DT, FAST> for the three mixed (GT, DT) -- a bf16
    gradient is FAST when (2W) % 8 == 0 ((8, 12), (20, 80), (16, 64)) and takes the plain packed loader at (8, 10); an fp32
    gradient into bf16 dx is FAST on all four"""
    from aide_amd import ops
    h, w = hw
    kx, ky = kinds
    x, dy, base, _, _ = S.up_case(2, 3, h, w)
    x16, dy16, base16 = x.bfloat16(), dy.bfloat16(), base.bfloat16()
    lx, ly = L(kx, x.shape), L(ky, dy.shape)
    ref = {}
    for xt in (FP, BF):                       # fp32 storage first: the reference of the widened input
        _, xv = lx.put(x16, dev, xt)
        for yt in (FP, BF):
            fy, yv = ly.blank(dev, yt)
            ops.upsample2x_fwd(xv, yv)
            if (xt, yt) == (FP, FP):
                ref['y'] = yv.clone()
                continue
            assert _bf16_allow(yv, ref['y'], yt == BF) and ly.intact(fy), 'forward %s -> %s' % (xt, yt)
    for acc in (False, True):
        for gt in (FP, BF):
            _, gv = ly.put(dy16, dev, gt)
            for dt in (FP, BF):
                fd, dv = lx.put(base16, dev, dt)
                ops.upsample2x_bwd(gv, dv, accumulate=acc)
                if (gt, dt) == (FP, FP):
                    ref[acc] = dv.clone()
                    continue
                assert _bf16_allow(dv, ref[acc], dt == BF) and lx.intact(fd), 'backward %s -> %s acc %s' % (gt, dt, acc)


@pytest.mark.parametrize('kinds', BF16_KINDS, ids='-'.join)
@pytest.mark.parametrize('k', [2, 5])
def test_bf16_head(dev, k, kinds):
    """head_fwd_kernel<K, bf16>, head_wgrad_kernel<K, bf16> (x bf16-stored) and head_dgrad_kernel<K, bf16> (dx bf16-stored),
    C = 64: bit-equal to the float instantiations on the widened x, dx narrowed RNE"""
    from aide_amd import ops
    kx, ky = kinds
    d = S.head_case(2, 64, k, 8, 12)
    x16 = d['x'].bfloat16()
    lx, ly = L(kx, x16.shape), L(ky, d['y'].shape)
    wd, bd = d['w'].to(dev), d['b'].to(dev)
    _, gv = ly.put(d['dy'], dev)
    res = {}
    for xt in (FP, BF):
        _, xv = lx.put(x16, dev, xt)
        fy, yv = ly.blank(dev)
        ops.head1x1_fwd(xv, wd, bd, yv)
        assert ly.intact(fy)
        out = [yv.clone()]
        for dt in (FP, BF):
            fd, dv = lx.blank(dev, dt)
            dw, db = torch.empty(k, 64, device=dev), torch.empty(k, device=dev)
            ops.head1x1_bwd(gv, xv, wd, dv, dw, db)
            assert lx.intact(fd)
            out += [dv.clone(), dw, db]
        res[xt] = out
    y32, dx32, dw32, db32 = res[FP][:4]
    S.assert_close(y32, S.head_ref(x16.float(), d['w'], d['b'], d['dy'])[0], HEAD_TOL, 'fp32 side, widened x')
    for xt in (FP, BF):
        y, dxa, dwa, dba, dxb, dwb, dbb = res[xt]
        assert torch.equal(y, y32) and torch.equal(dxa, dx32) and torch.equal(dxb, dx32.bfloat16())
        assert torch.equal(dwa, dw32) and torch.equal(dwb, dw32) and torch.equal(dba, db32) and torch.equal(dbb, db32)


@pytest.mark.parametrize('kind', ['dense', 'hi', 'lo'])
def test_bf16_fill(dev, kind):
    """a bf16 slice is zeroed as pairs by the fp32 kernels (fill_zero_kernel: C H W / 2 = 96 pairs)"""
    from aide_amd import ops
    lay = L(kind, (2, 4, 6, 8))
    flat, v = lay.blank(dev, BF)
    ops.fill_zero(v)
    assert float(v.float().abs().max()) == 0.0 and lay.intact(flat)


def test_mixed_entry_points_refuse_padded_strides(dev):
    """the bf16 entry points have no scalar fall-backs: layouts that the fp32 ones serve with them are AIDE_ERR_ARG"""
    from aide_amd import ops

    def mk(kind, shape, dt):
        return L(kind, shape).blank(dev, dt)

    for p in ('pad1', 'pad2'):
        fy, y = mk('dense', (2, 4, 4, 4), BF)
        with pytest.raises(RuntimeError):                                 # pool: x_bs % 4
            ops.maxpool2x2_fwd(mk(p, (2, 4, 8, 8), BF)[1], y)
        fd, dx = mk(p, (2, 4, 8, 8), BF)
        with pytest.raises(RuntimeError):                                 # pool backward: dx_bs % 4
            ops.maxpool2x2_bwd(mk('dense', (2, 4, 8, 8), FP)[1], mk('dense', (2, 4, 4, 4), FP)[1], dx)
        fu, u = mk(p, (2, 4, 16, 16), BF)
        with pytest.raises(RuntimeError):                                 # bilinear forward: y_bs % 4
            ops.upsample2x_fwd(mk('dense', (2, 4, 8, 8), FP)[1], u)
        torch.cuda.synchronize()
        assert all(bool((f == S.SENT).all()) for f in (fy, fd, fu))
    fy, y = mk('dense', (2, 4, 4, 3), BF)
    with pytest.raises(RuntimeError):                                     # pool: W % 4 (the fp32 entry point takes the scalar kernel)
        ops.maxpool2x2_fwd(mk('dense', (2, 4, 8, 6), BF)[1], y)
    fu, u = mk('dense', (2, 4, 6, 10), BF)
    with pytest.raises(RuntimeError):                                     # bilinear forward: odd W
        ops.upsample2x_fwd(mk('dense', (2, 4, 3, 5), FP)[1], u)
    fd, dx = mk('dense', (2, 4, 8, 8), FP)
    with pytest.raises(RuntimeError):                                     # bilinear backward: dy_bs odd (no gather kernel for bf16)
        ops.upsample2x_bwd(mk('pad1', (2, 4, 16, 16), BF)[1], dx)
    torch.cuda.synchronize()
    assert all(bool((f == S.SENT).all()) for f in (fy, fu, fd))
