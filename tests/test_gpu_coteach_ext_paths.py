"""Kernel-level net under the co-teaching extension kernels of csrc/coteach_ext.hip (-m gpu): the nine entry points on every
class count 2 .. 8, past the grid cap (more than 4096 x 256 elements) and past the droppixel grid (HW > 65536), on packed and
window region kernels with clipped, 1xK and Kx1 windows, and the selection on both sides of M = 1024, against the float64
references of tests/coteach_ext_cases.py (made binding on the host by tests/test_coteach_ext_reference_host.py).

The selection is kept out of every tolerance:
  1  maps and region-CE forward         through the C ABI against float64, at the bound
  2  aide_select_smallest               against the exact stable argsort of the same fp32 data: mask and ks bit-equal, sums within
                                        1e-12 relative of the float64 sum over the reference mask
  3  backward kernels                   through the C ABI with a prescribed seeded mask and coefficient 0.37 against float64
                                        autograd of coeff * sum(mask * map); every position the float64 gradient leaves at exactly
                                        0.0 (outside the mask, ignored region, not the arg-max of its window, image not in idx)
                                        is exactly 0.0
  4  the drop-in modules end to end     on operands that keep the k-th and (k + 1)-th selection value apart: masks exact, values
                                        and gradients dense at the bound
plus strided C-ABI calls in guarded buffers (bit-equal to dense, gaps and guards intact, every output word written),
determinism, saturated logits and the argument guards.

Bound: max |got - ref| <= 1e-4 max |ref| + 1e-9, the project's loss bound (loss_cases.rel_err); plain fp32 on the CPU needs at
most half of it on these inputs (test_coteach_ext_reference_host.py).  Run with -s for the largest error of each test.

Largest errors measured on an MI355X, in units of that bound: maps forward 0.002 (kl map, 3x46x50-c8); region-CE forward 0.001
(3x9x13-k4x4-c3); selection: mask and ks bit-equal, sums equal to the float64 sum (relative error 0.0 on all 20 cases);
prescribed-mask backward 0.014 (droppixel g, 3x1x1-c3) for the maps and 0.002 (3x46x50-k2x2-c5) for region CE; modules 0.003
(dropregionce, C = 8, scale 1, forget rate 0.5, grad2) and 0.011 (KLbidirection grad1, C = 8); saturated logits 0.019 (droppixel,
2x5x7-c8) and 0.002 (region dz, 3x6x8-k2x2-c8).  The strided C-ABI calls are bit-equal to the dense ones, whose errors these are.

Mutation check (not part of the suite; one change to coteach_ext.hip at a time, the 192 tests here and the six golden tests of the
same kernels in test_gpu_losses.py / test_gpu_multiclass.py):
  `v > best` -> `v >= best` in region_ce_win_kernel          37 test_region_ce_backward_prescribed_mask (every window case that
                                                             holds a tie) and 3 test_saturated_region_ce fail; no golden test
  `sel = rank < r_eq` -> `sel = true`                        17 test_select_smallest_exact fail (all but M = 1); no golden test,
                                                             test_select_smallest_ties_and_edges included
  the class-plane offset `+ c` dropped from one store of     20 test_maps_backward_prescribed_mask (every C >= 3 case), 2
  droppixel_bwd_mc_kernel (`g1[(n * C) * HW + p]`)           test_modules_pixel_selection, 2 test_saturated_maps fail; of the golden
                                                             tests test_golden_multiclass_rank4_operators (C = 3 and 5)
  `n * zb` -> `n * 2 * HW` in region_ce_bwd_kernel           test_abi_strided_region_ce_in_guarded_buffers[3x46x50-k2x2-c2] fails,
                                                             the one strided call of the packed two-class kernel; no golden test"""
import pytest
import torch

import loss_cases as LC
import coteach_ext_cases as X
from test_gpu_loss_paths import Slab, Worst

pytestmark = pytest.mark.gpu

DENSE = dict(a=0, b=0, t=0, g=0, h=0, s=0)
PADS = dict(a=24, b=40, t=56, g=8, h=72, s=24)        # a different pad per tensor (fp32 / int64 words per image)
SENTINEL = -7.0


class ByteSlab(Slab):
    """Slab of bytes (masks, aux buffers): n rows of `per` bytes, `pad` untouched bytes behind each, in the same NaN-patterned
    guarded buffer; the last word's spare bytes count as gap"""

    def __init__(self, dev, n, per, pad=0, src=None):
        self.per, self.bs, self.n = per, per + pad, n
        self.numel = (n * self.bs + 3) // 4
        self.buf, flat = LC.guarded(self.numel, LC.LEAD, dev)
        self.bytes = flat.view(torch.uint8)
        self.grid = self.bytes[:n * self.bs].view(n, self.bs)
        self.t = self.grid[:, :per]
        self.pattern = self.bytes.clone()
        if src is not None:
            self.t.copy_(src.reshape(n, per).to(dev))

    def intact(self):
        pat = self.pattern[:self.n * self.bs].view(self.n, self.bs)
        return LC.guards_intact(self.buf, LC.LEAD, self.numel) and torch.equal(self.grid[:, self.per:], pat[:, self.per:]) and \
            torch.equal(self.bytes[self.n * self.bs:], self.pattern[self.n * self.bs:])

    def fully_written(self, below=2):
        """no byte of the pattern (0xA5, 0xC5, 0x7F) is below 64: masks hold 0 / 1, packed aux bytes six bits"""
        return bool((self.t < below).all())


class Bufs(object):
    """the Slabs of one call sequence; pads: name of the pad class -> elements behind every row"""

    def __init__(self, dev, pads):
        self.dev, self.pads, self.all = dev, pads, []

    def _keep(self, name, s):
        self.all.append((name, s))
        return s

    def f32(self, name, rows, per, pad=None, src=None, dtype=torch.float32):
        return self._keep(name, Slab(self.dev, rows, per, self.pads[pad] if pad else 0, dtype, src))

    def i64(self, name, rows, per, pad=None, src=None):
        return self.f32(name, rows, per, pad, src, torch.int64)

    def u8(self, name, rows, per, pad=None, src=None):
        return self._keep(name, ByteSlab(self.dev, rows, per, self.pads[pad] if pad else 0, src))

    def scalar(self, name, value):
        return self.f32(name, 1, 1, src=torch.tensor([value]))

    def intact(self):
        for name, s in self.all:
            assert s.intact(), name                  # nothing written outside a view: not into a gap, not past either end


def _libs():
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    return lib, check, ptr, stream_ptr()


def _out(s):
    return s.t.contiguous().clone()


# ------------------------------------------------------------------------------------------------ the entry points, one by one
def run_kl(dev, case, pads, sat=False):
    """aide_kl_map forward, then backward with the reference's upstream map.  out and gout take no stride."""
    lib, check, ptr, sp = _libs()
    o = X.operands_of(case, sat)
    n, c, hw = case.n, case.c, case.h * case.w
    B = Bufs(dev, pads)
    z1, z2 = B.f32('z1', n, c * hw, 'a', o.z1), B.f32('z2', n, c * hw, 'b', o.z2)
    out = B.f32('out', 1, n * hw)
    check(lib.aide_kl_map(ptr(z1.t), z1.bs, ptr(z2.t), z2.bs, c, n, hw, ptr(out.t), None, None, 0, None, 0, sp), 'kl_map')
    gout = B.f32('gout', 1, n * hw, src=X.kl_reference(case, sat)[1])
    g1, g2 = B.f32('g1', n, c * hw, 'g'), B.f32('g2', n, c * hw, 'h')
    check(lib.aide_kl_map(ptr(z1.t), z1.bs, ptr(z2.t), z2.bs, c, n, hw, None, ptr(gout.t), ptr(g1.t), g1.bs, ptr(g2.t), g2.bs,
                          sp), 'kl_map bwd')
    torch.cuda.synchronize()
    B.intact()
    assert out.fully_written() and g1.fully_written() and g2.fully_written()
    return dict(out=_out(out), g1=_out(g1), g2=_out(g2))


def aux_written(aux, case):
    """every byte of the aux buffer, sized exactly by aide_region_ce_aux_bytes, is written: window kernels C + 1 ints per
    region (offsets below HW and a 17-bit target word: never the pattern), C-class words with bits 25 .. 31 clear (the
    pattern's top byte is 0x7F), two-class bytes of six bits"""
    if X.region_win(case.h, case.w, case.kh, case.kw) or case.c > 2:
        return not bool((aux.t.contiguous().view(torch.int32) == LC.NAN_BITS).any())
    return aux.fully_written(64)


def run_region(dev, case, pads, sat=False):
    """aide_region_ce_fwd, then aide_region_ce_bwd with the reference's mask.  loss, aux and mask take no stride."""
    lib, check, ptr, sp = _libs()
    z_, t_ = X.region_operands_of(case, sat)
    n, h, w, kh, kw, c = case
    total = X.region_count(n, h, w, kh, kw)
    B = Bufs(dev, pads)
    z, t = B.f32('z', n, c * h * w, 'a', z_), B.i64('t', n, h * w, 't', t_)
    nbytes = lib.aide_region_ce_aux_bytes(c, n, h, w, kh, kw)
    win = X.region_win(h, w, kh, kw)
    assert nbytes == total * ((c + 1) * 4 if win else 1 if c == 2 else 4)
    loss, aux = B.f32('loss', 1, total), B.u8('aux', 1, nbytes)
    check(lib.aide_region_ce_fwd(ptr(z.t), z.bs, ptr(t.t), t.bs, c, n, h, w, kh, kw, X.IGNORE, ptr(loss.t), ptr(aux.t), sp),
          'region_ce_fwd')
    mask = B.u8('mask', 1, total, src=X.region_reference(case, sat)[1])
    coeff = B.scalar('coeff', X.COEFF)
    dz = B.f32('dz', n, c * h * w, 'g')
    check(lib.aide_region_ce_bwd(ptr(z.t), z.bs, ptr(aux.t), ptr(mask.t), ptr(coeff.t), c, n, h, w, kh, kw, ptr(dz.t), dz.bs,
                                 sp), 'region_ce_bwd')
    torch.cuda.synchronize()
    B.intact()
    assert loss.fully_written() and aux_written(aux, case) and dz.fully_written()     # the windows tile the plane
    return dict(loss=_out(loss), aux=_out(aux), dz=_out(dz))


def run_select(dev, case, k_host, rr, k_in, only_positive):
    """aide_select_smallest on [nseg, stride] rows; the values past M of every row are NaN words the kernel must not read into
    the selection, the mask bytes past M stay untouched"""
    lib, check, ptr, sp = _libs()
    m, nseg, stride = case
    sel_, sum_ = X.select_values(case)
    B = Bufs(dev, dict(s=stride - m))
    sel, sums_in = B.f32('sel', nseg, m, 's', sel_[:, :m]), B.f32('sum_vals', nseg, m, 's', sum_[:, :m])
    mask = B.u8('mask', nseg, m, 's')
    sums, ks = B.f32('sums', 1, nseg, dtype=torch.float64), B.i64('ks', 1, nseg)
    kd = B.i64('k_in', 1, 1, src=torch.tensor([k_in])) if k_in is not None else None
    check(lib.aide_select_smallest(ptr(sel.t), ptr(sums_in.t), stride, nseg, m, int(k_host), float(rr),
                                   ptr(kd.t) if kd is not None else None, int(only_positive), ptr(mask.t), ptr(sums.t),
                                   ptr(ks.t), sp), 'select_smallest')
    torch.cuda.synchronize()
    B.intact()
    assert mask.fully_written() and sums.fully_written() and ks.fully_written()
    return _out(mask).cpu(), _out(sums).view(-1).cpu(), _out(ks).view(-1).cpu()


def run_droppixel(dev, case, idx, which, pads, sat=False):
    """aide_droppixel_map, then aide_droppixel_bwd with the reference's mask.  The gradients of the images in idx are pre-zeroed,
    as the contract asks; the images not in idx hold a sentinel, which must survive bit for bit: they are not written.  v,
    mask and the two gradient outputs take no stride."""
    lib, check, ptr, sp = _libs()
    o = X.operands_of(case, sat)
    n, c, hw, nd = case.n, case.c, case.h * case.w, len(idx)
    B = Bufs(dev, pads)
    z1, z2 = B.f32('z1', n, c * hw, 'a', o.z1), B.f32('z2', n, c * hw, 'b', o.z2)
    t, ix = B.i64('t', n, hw, 't', o.t), B.i64('idx', 1, nd, src=torch.tensor(idx))
    v = B.f32('v', 1, nd * hw)
    check(lib.aide_droppixel_map(ptr(z1.t), z1.bs, ptr(z2.t), z2.bs, ptr(t.t), t.bs, ptr(ix.t), nd, c, hw, which, X.IGNORE,
                                 ptr(v.t), sp), 'droppixel_map')
    mask = B.u8('mask', 1, nd * hw, src=X.droppixel_reference(case, idx, which, sat)[1])
    coeff = B.scalar('coeff', X.COEFF)
    g1, g2 = B.f32('g1', 1, n * c * hw), B.f32('g2', 1, n * c * hw)
    rest = [i for i in range(n) if i not in idx]
    for g in (g1, g2):
        g.t.zero_()
        g.t.view(n, c * hw)[rest] = SENTINEL
    check(lib.aide_droppixel_bwd(ptr(z1.t), z1.bs, ptr(z2.t), z2.bs, ptr(t.t), t.bs, ptr(ix.t), nd, c, hw, which, X.IGNORE,
                                 ptr(mask.t), ptr(coeff.t), ptr(g1.t), ptr(g2.t), sp), 'droppixel_bwd')
    torch.cuda.synchronize()
    B.intact()
    assert v.fully_written()
    for g in (g1, g2):
        assert bool((g.t.view(n, c * hw)[rest] == SENTINEL).all())
    return dict(v=_out(v), g1=_out(g1), g2=_out(g2))


def run_pixelcoreg(dev, case, three, pads, sat=False):
    """aide_pixelcoreg_map, then aide_pixelcoreg_bwd with the reference's mask.  Only the targets take a stride: the logits, the
    three maps, the mask and the gradients are dense by contract."""
    lib, check, ptr, sp = _libs()
    o = X.operands_of(case, sat)
    n, hw = case.n, case.h * case.w
    B = Bufs(dev, pads)
    z1, z2 = B.f32('z1', 1, n * 2 * hw, src=o.z1), B.f32('z2', 1, n * 2 * hw, src=o.z2)
    z3 = B.f32('z3', 1, n * 2 * hw, src=o.z3) if three else None
    t = B.i64('t', n, hw, 't', o.t)
    key, tf = B.f32('key', 1, n * hw), B.f32('tf', 1, n * hw)
    val = B.f32('val', 1, n * hw)
    p3 = ptr(z3.t) if three else None
    check(lib.aide_pixelcoreg_map(ptr(z1.t), ptr(z2.t), p3, ptr(t.t), t.bs, n, hw, X.KD, ptr(key.t),
                                  ptr(val.t) if three else None, ptr(tf.t), sp), 'pixelcoreg_map')
    mask = B.u8('mask', 1, n * hw, src=X.pixelcoreg_reference(case, three, X.KD, sat)[3])
    coeff = B.scalar('coeff', X.COEFF)
    res = {}
    if three:
        g3 = B.f32('g3', 1, n * 2 * hw)
        check(lib.aide_pixelcoreg_bwd(ptr(z1.t), ptr(z2.t), p3, ptr(t.t), t.bs, n, hw, X.KD, ptr(mask.t), ptr(coeff.t), None,
                                      None, ptr(g3.t), sp), 'pixelcoreg_bwd')
        outs = dict(val=val, g3=g3)
    else:
        g1, g2 = B.f32('g1', 1, n * 2 * hw), B.f32('g2', 1, n * 2 * hw)
        check(lib.aide_pixelcoreg_bwd(ptr(z1.t), ptr(z2.t), None, ptr(t.t), t.bs, n, hw, X.KD, ptr(mask.t), ptr(coeff.t),
                                      ptr(g1.t), ptr(g2.t), None, sp), 'pixelcoreg_bwd')
        outs = dict(g1=g1, g2=g2)
        assert LC.all_pattern(val.t)                 # val is written only with three nets
    outs.update(key=key, tf=tf)
    torch.cuda.synchronize()
    B.intact()
    for k, s in outs.items():
        assert s.fully_written(), k
        res[k] = _out(s)
    return res


def run_maps(dev, case, pads, sat=False):
    """every map entry point of a case -> dict name -> results"""
    res = {'kl': run_kl(dev, case, pads, sat)}
    for idx in X.droppixel_splits(case.n):
        for which in (0, 1):
            res['drop%s/%d' % (idx, which)] = run_droppixel(dev, case, idx, which, pads, sat)
    if case.c == 2:
        for three in (True, False):
            res['coreg%d' % three] = run_pixelcoreg(dev, case, three, pads, sat)
    return res


_CACHE = {}


def dense(fn, dev, case, *args):
    """the dense call's results, computed once and left unchanged"""
    key = (fn.__name__, case) + args
    if key not in _CACHE:
        _CACHE[key] = fn(dev, case, *(args + (DENSE,)))
    return _CACHE[key]


def zeros_hold(got, ref, what):
    assert X.structural_zeros_hold(got, ref), what + ': non-zero where the float64 gradient is exactly 0.0'


def compare_maps(w, res, case, sat=False, forward=True, backward=True):
    """groups 1 and 3 of the map kernels of one case against float64"""
    v, _, g1, g2 = X.kl_reference(case, sat)
    if forward:
        w.close(res['kl']['out'].view(v.shape), v, 'kl map')
    if backward:
        for k, g in (('g1', g1), ('g2', g2)):
            w.close(res['kl'][k].view(g.shape), g, 'kl ' + k)
            zeros_hold(res['kl'][k], g, 'kl ' + k)
    for idx in X.droppixel_splits(case.n):
        for which in (0, 1):
            r, name = res['drop%s/%d' % (idx, which)], 'droppixel %s which=%d' % (idx, which)
            v, _, g1, g2 = X.droppixel_reference(case, idx, which, sat)
            if forward:
                w.close(r['v'].view(v.shape), v, name)
            if backward:
                rest = [i for i in range(case.n) if i not in idx]
                for k, g in (('g1', g1), ('g2', g2)):
                    got = r[k].view(g.shape).clone()
                    assert bool((got[rest] == SENTINEL).all()) and not bool(g[rest].any()), name     # not written / no gradient
                    got[rest] = 0
                    w.close(got, g, '%s %s' % (name, k))
                    zeros_hold(got, g, name)
    if case.c == 2:
        for three in (True, False):
            r, name = res['coreg%d' % three], 'pixelcoreg three=%d' % three
            key, val, tf, _, grads = X.pixelcoreg_reference(case, three, X.KD, sat)
            if forward:
                w.close(r['key'].view(key.shape), key, name + ' key')
                assert torch.equal(r['tf'].view(tf.shape).cpu().double(), tf), name
                if three:
                    w.close(r['val'].view(val.shape), val, name + ' val')
            if backward:
                for k, g in zip(('g3',) if three else ('g1', 'g2'), grads):
                    w.close(r[k].view(g.shape), g, '%s %s' % (name, k))
                    zeros_hold(r[k], g, name)


# ------------------------------------------------------------------------------------------------ 1: forward against float64
@pytest.mark.parametrize('case', X.MAP_CASES, ids=X.map_id)
def test_maps_forward(dev, case):
    w = Worst('maps ' + X.map_id(case))
    compare_maps(w, dense(run_maps, dev, case), case, backward=False)
    w.report()


@pytest.mark.parametrize('case', X.REGION_CASES, ids=X.region_id)
def test_region_ce_forward(dev, case):
    """the loss of every region, 0.0 exactly where the region is ignored: pooled target 255, or no class in [0, C)"""
    w = Worst('region ' + X.region_id(case))
    v = X.region_reference(case)[0]
    got = dense(run_region, dev, case)['loss'].view(v.shape).cpu()
    w.close(got, v, 'loss')
    assert not bool(got[v == 0].any())
    w.report()


# ------------------------------------------------------------------------------------------------ 2: the selection, exactly
@pytest.mark.parametrize('case', X.SELECT_CASES, ids=X.select_id)
def test_select_smallest_exact(dev, case):
    from aide_amd.utils.coteach_loss import _select
    m, nseg, stride = case
    worst = 0.0
    for only_positive in (False, True):
        for k_host, rr, k_in in X.select_ks(case, only_positive):
            what = (k_host, rr, k_in, only_positive)
            mask, sums, ks = run_select(dev, case, k_host, rr, k_in, only_positive)
            rmask, rsums, rks = X.select_reference(case, k_host, rr, k_in, only_positive)
            assert torch.equal(ks, rks), what
            assert torch.equal(mask, rmask), (what, int((mask != rmask).sum()))
            err = ((sums - rsums).abs() / rsums.abs().clamp(min=1e-300)).max().item() if bool((rsums != 0).any()) else 0.0
            assert bool((sums[rsums == 0] == 0).all()) and err <= 1e-12, (what, err)
            worst = max(worst, err)
    if stride == m:         # and _select, the caller of the modules, is this dense call
        sel, sum_ = (x.to(dev).contiguous() for x in X.select_values(case))
        k_host, rr, k_in = X.select_ks(case, True)[2]
        mask, sums, ks = _select(sel, sum_, nseg, m, k_host=k_host, only_positive=True)
        rmask, rsums, rks = X.select_reference(case, k_host, -1.0, None, True)
        assert torch.equal(mask.cpu().view(nseg, m), rmask) and torch.equal(ks.cpu(), rks)
    print('select %-22s largest relative error of the sums %.2e' % (X.select_id(case), worst))


# ------------------------------------------------------------------------------------------------ 3: backward, prescribed mask
@pytest.mark.parametrize('case', X.MAP_CASES, ids=X.map_id)
def test_maps_backward_prescribed_mask(dev, case):
    w = Worst('maps bwd ' + X.map_id(case))
    compare_maps(w, dense(run_maps, dev, case), case, forward=False)
    w.report()


@pytest.mark.parametrize('case', X.REGION_CASES, ids=X.region_id)
def test_region_ce_backward_prescribed_mask(dev, case):
    w = Worst('region bwd ' + X.region_id(case))
    _, _, dz = X.region_reference(case)
    got = dense(run_region, dev, case)['dz'].view(dz.shape)
    w.close(got, dz, 'dz')
    zeros_hold(got, dz, 'dz')
    w.report()


# ------------------------------------------------------------------------------------------------ 4: the drop-in modules
def _mask_of(saved, i, ref):
    """saved[i] as the 0 / 1 byte mask it has to be, in the shape of the reference's"""
    m = saved[i]
    assert m.dtype == torch.uint8 and m.numel() == ref.numel() and int(m.max()) <= 1
    return m.cpu().view(ref.shape)


def _saved(loss, name):
    """the saved tensors of the first autograd node called `name` behind a loss.  The callers rely on the order of
    save_for_backward in aide_amd/utils: _RegionCEFn (z, aux, mask) -> [2]; _DropPixelFn (z1, z2, tg, idx, mask, ks) -> [4], [5];
    _PixelCoregFn (z1, z2, z3, tg, mask) -> [4].  Every mask is also checked for its dtype and size, so that a reordering fails
    here and does not compare another tensor."""
    todo, seen = [loss.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__.startswith(name):
            return f.saved_tensors
        todo.extend(g for g, _ in f.next_functions)
    return None


@pytest.mark.parametrize('c', X.MODULE_CLASSES)
def test_modules_region_ce(dev, c):
    """Coteachingloss_dropregionce at 2x2 (packed), 3x3, 4x4 and 1x1 windows: masks exact, both losses and gradients dense.  At
    forget rate 1.0 nothing is kept: the loss is NaN as in the reference (the mean of an empty set), its gradient 0."""
    from aide_amd import utils as U
    z1, z2, t = X.region_module_operands(c)
    w = Worst('dropregionce C=%d' % c)
    for scale in X.REGION_SCALES:
        for fr in X.FORGET_RATES:
            a1, a2 = z1.to(dev).requires_grad_(True), z2.to(dev).requires_grad_(True)
            l1, l2 = U.Coteachingloss_dropregionce(scale=scale, reduction='none')(a1, a2, t.to(dev), fr)
            ref = X.region_module_reference(z1, z2, t, scale, fr)
            what = 's=%g fr=%g' % (scale, fr)
            assert bool(torch.isnan(ref['loss1'])) == (fr == 1.0)
            for l, k in ((l1, '1'), (l2, '2')):
                assert torch.equal(_mask_of(_saved(l, '_RegionCEFn'), 2, ref['mask' + k]), ref['mask' + k]), what
                w.close(l, ref['loss' + k], '%s loss%s' % (what, k))
            l1.backward()
            assert a2.grad is None
            l2.backward()
            w.close(a1.grad, ref['grad1'], what + ' grad1')
            w.close(a2.grad, ref['grad2'], what + ' grad2')
    w.report()


@pytest.mark.parametrize('c', X.MODULE_CLASSES)
def test_modules_pixel_selection(dev, c):
    """KLbidirection, Coteachingloss_dropimagedroppixel and (two classes) both Pixelcoreg_Focalloss*: masks and pixel counts
    exact, values and gradients dense.  The two losses of the drop-pixel operator are back-propagated separately: the KL term
    reaches the other net."""
    from aide_amd import utils as U
    z1, z2, z3, t = X.pixel_module_operands(c)
    td = t.to(dev)
    w = Worst('pixel modules C=%d' % c)
    a1, a2 = z1.to(dev).requires_grad_(True), z2.to(dev).requires_grad_(True)
    v = U.KLbidirection(a1, a2)
    LC.backward_of(v)
    rv, (g1, g2) = X.masked_backward(X.kl_map, (z1, z2), LC.upstream(torch.zeros(v.shape, dtype=torch.float64)), 1.0)
    w.close(v, rv, 'KLbidirection')
    w.close(a1.grad, g1, 'KLbidirection grad1')
    w.close(a2.grad, g2, 'KLbidirection grad2')
    for fr in X.FORGET_RATES:
        ref = X.droppixel_module_reference(z1, z2, t, fr, 0.7)
        for which in (1, 2):
            a1, a2 = z1.to(dev).requires_grad_(True), z2.to(dev).requires_grad_(True)
            ls = U.Coteachingloss_dropimagedroppixel(weight=0.7, reduction='none')(a1, a2, td, fr)
            what = 'droppixel fr=%g loss%d' % (fr, which)
            saved = _saved(ls[which - 1], '_DropPixelFn')
            assert (saved is None) == (ref['mask%d' % which] is None), what
            if saved is not None:
                assert torch.equal(_mask_of(saved, 4, ref['mask%d' % which]), ref['mask%d' % which]), what
                assert saved[5].dtype == torch.int64 and int(saved[5][0]) == int(ref['mask%d' % which].sum()), what
            w.close(ls[which - 1], ref['loss%d' % which], what)
            # NaN as in the reference: nothing kept at forget rate 1.0, or no foreground among the dropped images (C = 2, 0.25)
            assert bool(torch.isnan(ref['loss%d' % which])) == (fr == 1.0 or ref.get('count%d' % which) == 0), what
            ls[which - 1].backward()
            for k, x in ((1, a1), (2, a2)):
                g = torch.zeros_like(x) if x.grad is None else x.grad
                w.close(g, ref['l%d_grad%d' % (which, k)], '%s grad%d' % (what, k))
    if c == 2:
        for three in (True, False):
            for fr, kd, red in ((0.0, 0.3, 'mean'), (0.25, 0.3, 'mean'), (0.5, 0.7, 'sum'), (0.25, 0.7, 'sum'), (0.5, 0.3, 'mean'),
                                (1.0, 0.3, 'mean'), (1.0, 0.7, 'sum')):
                zs = [z.to(dev).requires_grad_(True) for z in ((z1, z2, z3) if three else (z1, z2))]
                op = U.Pixelcoreg_Focalloss if three else U.Pixelcoreg_Focalloss_twomodel
                loss, frac = op(reduction=red)(*zs, td, fr, kd, dev)
                ref = X.pixelcoreg_module_reference(z1, z2, z3 if three else None, t, fr, kd, red)
                what = 'pixelcoreg three=%d fr=%g kd=%g %s' % (three, fr, kd, red)
                assert torch.equal(_mask_of(_saved(loss, '_PixelCoregFn'), 4, ref['mask']), ref['mask']), what
                w.close(loss, ref['loss'], what)
                w.close(frac, ref['frac'], what + ' frac')
                loss.backward()
                if three:
                    assert zs[0].grad is None and zs[1].grad is None
                for x, g in zip(zs[2:] if three else zs, ref['grads']):
                    w.close(x.grad, g, what + ' grad')
    w.report()


# ------------------------------------------------------------------------------------------------ the strided C ABI
@pytest.mark.parametrize('case', [X.MapCase(3, 46, 50, c) for c in (2, 4, 7)], ids=X.map_id)
def test_abi_strided_maps_in_guarded_buffers(dev, case):
    """batch strides larger than dense on every tensor that takes one (b1, b2, gb1, gb2, tb), a different pad per tensor, every
    tensor a view into a NaN-patterned guarded buffer: bit for bit the dense call; gaps and guards intact and every output word
    written (asserted inside the run_* helpers).  aide_pixelcoreg_* take a stride for the targets only and the gradient outputs
    of aide_droppixel_bwd none: those tensors are dense in both runs."""
    assert case in X.MAP_CASES
    ref, res = dense(run_maps, dev, case), run_maps(dev, case, PADS)
    assert sorted(ref) == sorted(res)
    for name in ref:
        for k, v in ref[name].items():
            assert torch.equal(v.view(torch.int32), res[name][k].view(torch.int32)), (name, k)


@pytest.mark.parametrize('case', X.REGION_ABI_CASES, ids=X.region_id)
def test_abi_strided_region_ce_in_guarded_buffers(dev, case):
    """zb, tb and db larger than dense; the aux buffer sized exactly by aide_region_ce_aux_bytes and all of it written"""
    ref, res = dense(run_region, dev, case), run_region(dev, case, PADS)
    for k, v in ref.items():
        assert torch.equal(v.view(torch.uint8), res[k].view(torch.uint8)), k


# ------------------------------------------------------------------------------------------------ determinism, saturation
def test_determinism(dev):
    """two runs of every entry point are bit-identical at a multi-block case (no atomics on floating-point data; the
    selection's shared-memory histogram counts integers)"""
    case = X.MAP_MULTI_BLOCK
    a, b = run_maps(dev, case, DENSE), run_maps(dev, case, DENSE)
    c2 = X.MapCase(case.n, case.h, case.w, 2)
    a.update(('c2 ' + k, v) for k, v in run_maps(dev, c2, DENSE).items() if k.startswith('coreg'))
    b.update(('c2 ' + k, v) for k, v in run_maps(dev, c2, DENSE).items() if k.startswith('coreg'))
    for rc in (X.RegionCase(*(g + (5,))) for g in X.REGION_MULTI_BLOCK):
        a['region ' + X.region_id(rc)], b['region ' + X.region_id(rc)] = run_region(dev, rc, DENSE), run_region(dev, rc, DENSE)
    assert any(k.startswith('c2 coreg') for k in a)
    for name in a:
        for k, v in a[name].items():
            assert torch.equal(v.view(torch.uint8), b[name][k].view(torch.uint8)), (name, k)
    sc = X.SelectCase(5000, 3, 5024)
    form = X.select_ks(sc, True)[2]
    for x, y in zip(run_select(dev, sc, *(form + (True,))), run_select(dev, sc, *(form + (True,)))):
        assert torch.equal(x, y)


@pytest.mark.parametrize('case', X.SATURATION_CASES, ids=X.map_id)
def test_saturated_maps(dev, case):
    """logit differences of +-80: soft-max terms under- and overflow towards 0 and 1; maps and gradients stay finite and within
    the bound"""
    res = run_maps(dev, case, DENSE, True)
    for name in res:
        for k, v in res[name].items():
            assert bool(torch.isfinite(v).all()), (name, k)
    w = Worst('saturated ' + X.map_id(case))
    compare_maps(w, res, case, True)
    w.report()


@pytest.mark.parametrize('case', X.REGION_SATURATION_CASES, ids=X.region_id)
def test_saturated_region_ce(dev, case):
    assert case in X.REGION_CASES
    res = run_region(dev, case, DENSE, True)
    v, _, dz = X.region_reference(case, True)
    assert bool(torch.isfinite(res['loss']).all()) and bool(torch.isfinite(res['dz']).all())
    w = Worst('saturated region ' + X.region_id(case))
    w.close(res['loss'].view(v.shape), v, 'loss')
    w.close(res['dz'].view(dz.shape), dz, 'dz')
    zeros_hold(res['dz'], dz, 'dz')
    w.report()


# ------------------------------------------------------------------------------------------------ argument guards
def test_argument_guards(dev):
    """a class count outside 2 .. 8, ndrop = 0, M = 0 and a missing output pointer: a negative code, nothing launched, the
    pre-filled outputs unchanged (the pattern of test_class_count_limits)"""
    lib, _, ptr, sp = _libs()
    n, h, w = 2, 8, 8
    hw = h * w
    z = torch.randn(n, 9, h, w, device=dev)
    t = torch.zeros(n, h, w, dtype=torch.long, device=dev)
    fill = lambda k, dtype=torch.float32: torch.full((k,), SENTINEL, dtype=dtype, device=dev)
    bytes_ = lambda k: torch.full((k,), 0xA5, dtype=torch.uint8, device=dev)
    outs = []

    def keep(x):
        outs.append((x, x.clone()))
        return x

    idx, coeff = torch.tensor([1], device=dev), torch.tensor([1.0], device=dev)
    mask = torch.ones(n * hw, dtype=torch.uint8, device=dev)
    gm = mask.float()
    for c in (1, 9):
        zc = z[:, :c].contiguous()
        assert lib.aide_kl_map(ptr(zc), c * hw, ptr(zc), c * hw, c, n, hw, ptr(keep(fill(n * hw))), None, None, 0, None, 0, sp) < 0
        assert lib.aide_kl_map(ptr(zc), c * hw, ptr(zc), c * hw, c, n, hw, None, ptr(gm), ptr(keep(fill(n * c * hw))),
                               c * hw, ptr(keep(fill(n * c * hw))), c * hw, sp) < 0
        assert lib.aide_region_ce_aux_bytes(c, n, h, w, 2, 2) == 0 and lib.aide_region_ce_aux_bytes(c, n, h, w, 3, 3) == 0
        for k in (2, 3):
            aux = keep(bytes_(n * hw * 40))
            assert lib.aide_region_ce_fwd(ptr(zc), c * hw, ptr(t), hw, c, n, h, w, k, k, 255, ptr(keep(fill(n * hw))), ptr(aux),
                                          sp) < 0
            assert lib.aide_region_ce_bwd(ptr(zc), c * hw, ptr(aux), ptr(mask), ptr(coeff), c, n, h, w, k, k,
                                          ptr(keep(fill(n * c * hw))), c * hw, sp) < 0
        assert lib.aide_droppixel_map(ptr(zc), c * hw, ptr(zc), c * hw, ptr(t), hw, ptr(idx), 1, c, hw, 0, 255,
                                      ptr(keep(fill(hw))), sp) < 0
        assert lib.aide_droppixel_bwd(ptr(zc), c * hw, ptr(zc), c * hw, ptr(t), hw, ptr(idx), 1, c, hw, 0, 255, ptr(mask),
                                      ptr(coeff), ptr(keep(fill(n * c * hw))), ptr(keep(fill(n * c * hw))), sp) < 0
    z2 = z[:, :2].contiguous()
    # ndrop = 0
    assert lib.aide_droppixel_map(ptr(z2), 2 * hw, ptr(z2), 2 * hw, ptr(t), hw, ptr(idx), 0, 2, hw, 0, 255, ptr(keep(fill(hw))),
                                  sp) < 0
    assert lib.aide_droppixel_bwd(ptr(z2), 2 * hw, ptr(z2), 2 * hw, ptr(t), hw, ptr(idx), 0, 2, hw, 0, 255, ptr(mask), ptr(coeff),
                                  ptr(keep(fill(n * 2 * hw))), ptr(keep(fill(n * 2 * hw))), sp) < 0
    # M = 0, no segment
    v = torch.rand(64, device=dev)
    for nseg, m in ((1, 0), (0, 64)):
        assert lib.aide_select_smallest(ptr(v), ptr(v), 64, nseg, m, 3, -1.0, None, 0, ptr(keep(bytes_(64))),
                                        ptr(keep(fill(1, torch.float64))), ptr(keep(fill(1, torch.int64))), sp) < 0
    # a missing output pointer
    assert lib.aide_kl_map(ptr(z2), 2 * hw, ptr(z2), 2 * hw, 2, n, hw, None, None, None, 0, None, 0, sp) < 0
    assert lib.aide_kl_map(ptr(z2), 2 * hw, ptr(z2), 2 * hw, 2, n, hw, None, ptr(gm), ptr(keep(fill(n * 2 * hw))), 2 * hw,
                           None, 2 * hw, sp) < 0
    aux = keep(bytes_(n * hw * 40))
    assert lib.aide_region_ce_fwd(ptr(z2), 2 * hw, ptr(t), hw, 2, n, h, w, 2, 2, 255, None, ptr(aux), sp) < 0
    assert lib.aide_region_ce_fwd(ptr(z2), 2 * hw, ptr(t), hw, 2, n, h, w, 2, 2, 255, ptr(keep(fill(n * hw))), None, sp) < 0
    assert lib.aide_region_ce_bwd(ptr(z2), 2 * hw, ptr(aux), ptr(mask), ptr(coeff), 2, n, h, w, 2, 2, None, 2 * hw, sp) < 0
    assert lib.aide_select_smallest(ptr(v), ptr(v), 64, 1, 64, 3, -1.0, None, 0, None, ptr(keep(fill(1, torch.float64))),
                                    ptr(keep(fill(1, torch.int64))), sp) < 0
    assert lib.aide_select_smallest(ptr(v), ptr(v), 64, 1, 64, 3, -1.0, None, 0, ptr(keep(bytes_(64))), None,
                                    ptr(keep(fill(1, torch.int64))), sp) < 0
    assert lib.aide_droppixel_map(ptr(z2), 2 * hw, ptr(z2), 2 * hw, ptr(t), hw, ptr(idx), 1, 2, hw, 0, 255, None, sp) < 0
    assert lib.aide_droppixel_bwd(ptr(z2), 2 * hw, ptr(z2), 2 * hw, ptr(t), hw, ptr(idx), 1, 2, hw, 0, 255, ptr(mask), ptr(coeff),
                                  ptr(keep(fill(n * 2 * hw))), None, sp) < 0
    assert lib.aide_pixelcoreg_map(ptr(z2), ptr(z2), None, ptr(t), hw, n, hw, 0.3, None, None, ptr(keep(fill(n * hw))), sp) < 0
    assert lib.aide_pixelcoreg_map(ptr(z2), ptr(z2), ptr(z2), ptr(t), hw, n, hw, 0.3, ptr(keep(fill(n * hw))), None,
                                   ptr(keep(fill(n * hw))), sp) < 0           # three nets need val
    assert lib.aide_pixelcoreg_bwd(ptr(z2), ptr(z2), None, ptr(t), hw, n, hw, 0.3, ptr(mask), ptr(coeff),
                                   ptr(keep(fill(n * 2 * hw))), None, None, sp) < 0
    assert lib.aide_pixelcoreg_bwd(ptr(z2), ptr(z2), ptr(z2), ptr(t), hw, n, hw, 0.3, ptr(mask), ptr(coeff),
                                   ptr(keep(fill(n * 2 * hw))), ptr(keep(fill(n * 2 * hw))), None, sp) < 0
    torch.cuda.synchronize()
    for x, before in outs:
        assert torch.equal(x.view(torch.uint8), before.view(torch.uint8))
