"""References, layouts and inputs of tests/test_gpu_spatial_head.py (max-pool 2x2, bilinear x2, the 1x1 head, zero fill),
validated without a GPU by tests/test_spatial_reference_host.py.  Everything here is plain torch on the CPU:

  * max-pool: aten's max_pool2d and its autograd on the same fp32 values (exact), plus an explicit statement of the
    first-maximum tie rule (pool_first_max) that the host test holds aten to;
  * bilinear x2 (align_corners=True): y = Rh x Rw^T and dx = Rh^T dy Rw in float64, the interpolation matrices built from
    fp32-computed indices and weights as aten and src_index (spatial.hip) compute them -- a float64 F.interpolate is NOT
    this operator: its indices differ from the fp32 ones by up to 3.2e-5 of the output scale at W ~ 510;
  * head: float64 F.conv2d with a 1x1 filter and its autograd; the _bn forms on relu(z * scale[c] + shift[c]) in float64.

Layout: an NCHW tensor as a view of a flat, sentinel-filled allocation (guard elements on both sides), so that a test can
assert that a kernel wrote nothing but the planes it was given."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SENT = -768.0          # sentinel: exact in fp32 and bf16, far from every value the cases produce
GUARD = 64             # elements before and after the view (a multiple of 16 bytes in either storage type)
KINDS = ('dense', 'lo', 'hi', 'pad1', 'pad2', 'pad4')


# ------------------------------------------------------------------------------------------------ layouts
class Layout(object):
    """An [N, C, H, W] view with dense channel planes inside a flat allocation:
       dense       batch stride C*H*W
       lo / hi     channels [0, C) / [C, 2C) of a contiguous 2C-channel buffer: batch stride 2*C*H*W (concat buffers)
       pad1/2/4    batch stride C*H*W + 1 / 2 / 4 (an as_strided view; needs N >= 2 to matter)"""

    def __init__(self, kind, shape):
        assert kind in KINDS
        n, c, h, w = shape
        chw = c * h * w
        self.kind, self.shape = kind, tuple(shape)
        self.offset = GUARD + (chw if kind == 'hi' else 0)
        if kind in ('lo', 'hi'):
            self.bs = 2 * chw
        elif kind == 'dense':
            self.bs = chw
        else:
            self.bs = chw + int(kind[3:])
        self.strides = (self.bs, h * w, w, 1)
        span = n * 2 * chw if kind in ('lo', 'hi') else (n - 1) * self.bs + chw
        self.numel = GUARD + span + GUARD

    def alloc(self, device, dtype=torch.float32):
        return torch.full((self.numel,), SENT, dtype=dtype, device=device)

    def view(self, flat):
        return flat.as_strided(self.shape, self.strides, self.offset)

    def blank(self, device, dtype=torch.float32):
        """-> (flat, view), sentinel everywhere (the view included: an element the kernel skips shows up as SENT)"""
        flat = self.alloc(device, dtype)
        return flat, self.view(flat)

    def put(self, value, device, dtype=torch.float32):
        """-> (flat, view) with `value` copied into the view"""
        flat, v = self.blank(device, dtype)
        v.copy_(value.to(device=device, dtype=dtype))
        return flat, v

    def intact(self, flat):
        """every element of the allocation outside the view still holds the sentinel"""
        f = flat.clone()
        self.view(f).fill_(SENT)
        return bool((f == SENT).all())


def rel_err(got, ref):
    """max |got - ref| / max |ref| in float64"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-30)


def assert_close(got, ref, rtol, what=''):
    err = rel_err(got, ref)
    assert err <= rtol, '%s: max abs err %.3e of the reference scale > %.3e' % (what, err, rtol)


# ------------------------------------------------------------------------------------------------ max-pool
def pool_input(n, c, h, w, seed=0):
    """values on a coarse grid (ties in most windows), then per channel (index mod 5):
       0  a constant plane: whole windows equal        1  odd rows repeat the even rows: ties across the two window rows
       2  negative values only                          3  image 0: -inf, the others: +0.0 / -0.0 at random
       4  left as drawn"""
    g = torch.Generator().manual_seed(1000 + seed + 7 * h + w)
    x = torch.randint(-3, 4, (n, c, h, w), generator=g).float() * 0.5
    for ch in range(c):
        k = ch % 5
        if k == 0:
            x[:, ch] = 0.25
        elif k == 1:
            x[:, ch, 1::2] = x[:, ch, 0::2]
        elif k == 2:
            x[:, ch] = -x[:, ch].abs() - 0.5
        elif k == 3:
            sign = torch.randint(0, 2, (n, h, w), generator=g).float() * 2.0 - 1.0
            x[:, ch] = torch.copysign(torch.zeros(n, h, w), sign)
            x[0, ch] = float('-inf')
    return x


def pool_ref(x, dy):
    """(y, dx) of F.max_pool2d(x, 2, 2) and its autograd"""
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2, 2)
    y.backward(dy)
    return y.detach(), xr.grad


def pool_first_max(x, dy):
    """the same, written out: the maximum of the window in row-major order, the gradient to the FIRST element that
    attains it (`val > max` moves the arg-max, equality does not; +0.0 == -0.0)"""
    win = [x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]]
    m, k = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.long)
    for j in (1, 2, 3):
        better = win[j] > m
        m = torch.where(better, win[j], m)
        k = torch.where(better, torch.full_like(k, j), k)
    dx = torch.zeros_like(x)
    for j in range(4):
        dx[..., j // 2::2, j % 2::2] = torch.where(k == j, dy, torch.zeros_like(dy))
    return m, dx


@functools.lru_cache(maxsize=None)
def pool_case(n, c, h, w):
    """-> x, dy, base (what the accumulating backward adds onto), y_ref, dx_ref: fp32 on the CPU, computed once"""
    g = torch.Generator().manual_seed(31 * h + w)
    x = pool_input(n, c, h, w)
    dy = torch.randn(n, c, h // 2, w // 2, generator=g)
    base = torch.randn(n, c, h, w, generator=g)
    y, dx = pool_ref(x, dy)
    return x, dy, base, y, dx


# ------------------------------------------------------------------------------------------------ bilinear x2
@functools.lru_cache(maxsize=None)
def interp_matrix(n_in):
    """R [2 n_in, n_in] in float64 with the fp32 index arithmetic of aten (UpSample.h, align_corners=True) and src_index:
    scale = float32(in - 1) / float32(out - 1), src = float32(scale * dst), i0 = min(int(src), in - 1),
    i1 = i0 + (i0 < in - 1), l1 = float32(src - i0), l0 = float32(1 - l1)"""
    n_out = 2 * n_in
    r = np.zeros((n_out, n_in), dtype=np.float64)
    scale = np.float32(n_in - 1) / np.float32(n_out - 1)
    for dst in range(n_out):
        src = np.float32(scale * np.float32(dst))
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = np.float32(src - np.float32(i0))
        l0 = np.float32(np.float32(1.0) - l1)
        r[dst, i0] += float(l0)
        r[dst, i1] += float(l1)
    return torch.from_numpy(r)


def upsample_ref(x):
    """float64 y [N, C, 2H, 2W] = Rh x Rw^T"""
    rh, rw = interp_matrix(x.shape[2]), interp_matrix(x.shape[3])
    return torch.matmul(torch.matmul(rh, x.double()), rw.t())


def upsample_bwd_ref(dy):
    """float64 dx [N, C, H, W] = Rh^T dy Rw"""
    rh, rw = interp_matrix(dy.shape[2] // 2), interp_matrix(dy.shape[3] // 2)
    return torch.matmul(torch.matmul(rh.t(), dy.double()), rw)


@functools.lru_cache(maxsize=None)
def up_case(n, c, h, w):
    """-> x, dy, base (fp32), y_ref, dx_ref (float64): computed once"""
    g = torch.Generator().manual_seed(977 * h + w)
    x = torch.randn(n, c, h, w, generator=g)
    dy = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    base = torch.randn(n, c, h, w, generator=g)
    return x, dy, base, upsample_ref(x), upsample_bwd_ref(dy)


# ------------------------------------------------------------------------------------------------ head
def head_ref(x, w, b, dy, scale=None, shift=None):
    """float64 (logits, dx, dw [K, C], db) of conv2d(a, w [K, C], b) with a = x, or relu(x * scale[c] + shift[c]) for the
    _bn forms (dx is then the gradient with respect to a); b may be None (db is None)"""
    a = x.double()
    if scale is not None:
        a = torch.relu(a * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    k, c = w.shape
    ar = a.clone().requires_grad_(True)
    wr = w.double().view(k, c, 1, 1).clone().requires_grad_(True)
    br = b.double().clone().requires_grad_(True) if b is not None else None
    y = F.conv2d(ar, wr, br)
    y.backward(dy.double())
    return y.detach(), ar.grad, wr.grad.view(k, c), (br.grad if br is not None else None)


@functools.lru_cache(maxsize=None)
def head_case(n, c, k, h, w, bn=False):
    """-> dict of fp32 inputs (x, w, b, dy, scale, shift) and float64 references (y, y_nobias, dx, dw, db): computed once.
    bn: mixed-sign scale / shift, so that about half of the activations are clipped"""
    g = torch.Generator().manual_seed(100 * k + c + (5000 if bn else 0))
    d = dict(x=torch.randn(n, c, h, w, generator=g), w=torch.randn(k, c, generator=g) * (1.0 / c ** 0.5),
             b=torch.randn(k, generator=g), dy=torch.randn(n, k, h, w, generator=g), scale=None, shift=None)
    if bn:
        d['scale'] = torch.randn(c, generator=g)
        d['shift'] = torch.randn(c, generator=g) * 0.5
    d['y'], d['dx'], d['dw'], d['db'] = head_ref(d['x'], d['w'], d['b'], d['dy'], d['scale'], d['shift'])
    d['y_nobias'] = d['y'] - d['b'].double().view(1, k, 1, 1)
    return d
