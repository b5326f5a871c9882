"""Shared by test_coteach_ext_reference_host.py and test_gpu_coteach_ext_paths.py: the cases of the co-teaching extension kernels
(csrc/coteach_ext.hip), their operands and float64 references written out from the header comments of coteach_ext.hip and from
oracle/losses.py.  Everything here is plain torch on the CPU; no library call and no golden file.

MAP_CASES          MapCase(n, h, w, c) of the per-pixel maps (kl_map*, pixelcoreg_map, droppixel_map*) and their backwards
REGION_CASES       RegionCase(n, h, w, kh, kw, c) of the max-pooled region cross entropy; region_win() / grid_blocks() restate the
                   library's dispatch and grid cap, test_coteach_ext_reference_host.py asserts that every path keeps its case
SELECT_CASES       SelectCase(m, nseg, stride) of the k-smallest selection; select_values() / select_ks() are the data and the k
                   forms, select_reference() the exact stable-argsort reference
*_reference        float64, every input upcast first, one plain autograd pass each
MODULE_*           the drop-in modules end to end on inputs that obey a gap rule, so that masks compare exactly"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import loss_cases as LC

IGNORE = LC.IGNORE
BLOCK, GRID_CAP = 256, 4096                # grid1(): min(ceil(total / 256), 4096) blocks of 256 threads (coteach_ext.hip, `int grid1`)
DROPPIXEL_CAP = 256                        # aide_droppixel_*: dim3 grid(min(ceil(HW / 256), 256), ndrop)
SELECT_THREADS = 1024                      # select_smallest_kernel: one workgroup per segment, cpt = ceil(M / 1024)
CLASS_COUNTS = tuple(range(2, 9))
COEFF = 0.37                               # the coefficient of the prescribed-mask backward calls: not 1
MASK_SHARE = 0.6
FORGET_RATES = (0.0, 0.25, 0.5, 1.0)


def _seed(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------- the per-pixel maps
MapCase = collections.namedtuple('MapCase', 'n h w c')
# (N, H, W): HW = 1 (255 idle threads), 35 (less than a wavefront), 2300 x 3 = 6900 pixels (27 blocks, ragged tail; 9 droppixel
# blocks per image)
MAP_SMALL = ((3, 1, 1), (2, 5, 7), (3, 46, 50))
# HW = 66564 > 256 * 256: the blockIdx.x stride of the droppixel kernels, ragged tail;
# 1,052,676 pixels > 4096 * 256: the grid1 stride of the kl / pixelcoreg kernels, ragged tail (4100 pixels in the second stride)
MAP_LARGE = (((2, 258, 258), (2, 5)), ((1, 1026, 1026), (2, 3)))
MAP_CASES = tuple(MapCase(n, h, w, c) for (n, h, w) in MAP_SMALL for c in CLASS_COUNTS) + \
    tuple(MapCase(n, h, w, c) for (n, h, w), cs in MAP_LARGE for c in cs)
MAP_MULTI_BLOCK = MapCase(3, 46, 50, 5)
SATURATION_CASES = tuple(MapCase(2, 5, 7, c) for c in (2, 3, 8))
KD = 0.3                                   # the kdweight of the map-level pixelcoreg calls


def map_id(c):
    return '%dx%dx%d-c%d' % c


MapOperands = collections.namedtuple('MapOperands', 'z1 z2 z3 t')


@functools.lru_cache(maxsize=None)
def map_operands(case):
    """fp32 logits of two nets (the second correlated with the first, so that KL and CE are of one size) and of a third for
    Pixelcoreg_Focalloss (two classes only); targets uniform in [0, C) with an ignored stretch in image 0 and, where there is
    room, one label C + 2 that is no class"""
    n, h, w, c = case
    g = _seed('map-' + map_id(case))
    z1 = torch.randn(n, c, h, w, generator=g) * 2
    z2 = (0.6 * z1 + torch.randn(n, c, h, w, generator=g) * 1.5).contiguous()
    z3 = torch.randn(n, c, h, w, generator=g) * 2 if c == 2 else None
    t = torch.randint(0, c, (n, h, w), generator=g)
    if w >= 5:
        t[0, 0, :5] = IGNORE
        t[0, 1, 1] = c + 2
    return MapOperands(z1, z2, z3, t)


def saturated(case):
    """both nets' logits of the case scaled so that differences between classes reach +-80 (the idea of loss_cases.saturated)"""
    o = map_operands(case)
    out = []
    for k, z in enumerate((o.z1, o.z2)):
        zs = z * (80.0 / (z.max() - z.min()).item())
        a, b = (40.0, -40.0) if k == 0 else (-40.0, 40.0)
        zs[0, 0, 0, 0], zs[0, 1, 0, 0] = a, b
        zs[0, 0, 0, 1], zs[0, 1, 0, 1] = b, a
        out.append(zs.contiguous())
    return o._replace(z1=out[0], z2=out[1], z3=out[0].flip(0).contiguous() if o.z3 is not None else None)


def operands_of(case, sat=False):
    return saturated(case) if sat else map_operands(case)


def kl_map(z1, z2):
    """sum_c (p1_c - p2_c)(l1_c - l2_c), l = log-soft-max: KL(p1 || p2) + KL(p2 || p1) -> [N, H, W]"""
    l1, l2 = torch.log_softmax(z1, 1), torch.log_softmax(z2, 1)
    return ((l1.exp() - l2.exp()) * (l1 - l2)).sum(1)


def droppixel_class(t, c):
    """the class of the CE term of the drop-pixel map and where it is on.  Two classes: every non-zero target is class 1.
    C classes: off where the target is ignore_index or no class in (0, C) (the header of droppixel_map_mc_kernel); the map is
    target * (...), so class 0 never counts."""
    if c == 2:
        return (t != 0).long()
    on = (t != IGNORE) & (t > 0) & (t < c)
    return torch.where(on, t, torch.full_like(t, IGNORE))


def droppixel_map(z1, z2, t, idx, which):
    """v[m] = target * (KL(z1, z2) + CE(z_which, target)) on the images idx[m] -> [ndrop, H, W]"""
    idx = torch.as_tensor(idx)
    a, b, tt = z1[idx], z2[idx], t[idx]
    ce = F.cross_entropy(b if which else a, droppixel_class(tt, z1.shape[1]), ignore_index=IGNORE, reduction='none')
    return tt.to(z1.dtype) * (kl_map(a, b) + ce)


def focal(z, tg):
    """focal(gamma = 2) cross entropy of two-class logits against tg in {0, 1} (utils/reg_loss.py:69-97)"""
    l, q = torch.log_softmax(z, 1), torch.softmax(z, 1)
    return -tg * (1 - q[:, 1]) ** 2 * l[:, 1] - (1 - tg) * (1 - q[:, 0]) ** 2 * l[:, 0]


def pixelcoreg_maps(z1, z2, z3, t, kd):
    """-> (key, val, tf): key = (1 - kd) sum of the nets' focal terms + kd KL(1, 2); val = focal of net 3, or the key with two
    nets; tf = the target as 0 / 1 (every non-zero target is foreground)"""
    tg = (t != 0).to(z1.dtype)
    fs = [focal(z, tg) for z in (z1, z2) + ((z3,) if z3 is not None else ())]
    key = (1 - kd) * sum(fs) + kd * kl_map(z1, z2)
    return key, (fs[2] if z3 is not None else key), tg


def seeded_mask(name, shape):
    return (torch.rand(shape, generator=_seed('mask-' + name)) < MASK_SHARE).to(torch.uint8)


def masked_backward(value_fn, inputs, mask, coeff=COEFF, dtype=torch.float64):
    """float64 autograd of coeff * sum(mask * value_fn(*inputs)) -> (value map, gradients of the inputs)"""
    leaves = [x.detach().to(dtype).clone().requires_grad_(True) for x in inputs]
    v = value_fn(*leaves)
    (coeff * (mask.to(dtype).reshape(v.shape) * v).sum()).backward()
    return v.detach(), [x.grad if x.grad is not None else torch.zeros_like(x) for x in leaves]


@functools.lru_cache(maxsize=None)
def kl_reference(case, sat=False):
    """-> (map, upstream gradient, d z1, d z2): the upstream is COEFF on a seeded mask, exactly 0 elsewhere"""
    o = operands_of(case, sat)
    gout = seeded_mask('kl-' + map_id(case), o.t.shape).float() * COEFF
    v, (g1, g2) = masked_backward(kl_map, (o.z1, o.z2), gout, 1.0)
    return v, gout, g1, g2


def droppixel_splits(n):
    """(idx, ...) for ndrop = 1 and N - 1, unordered"""
    return {1: ((0,),), 2: ((1,), (0,)), 3: ((1,), (2, 0))}[n]


@functools.lru_cache(maxsize=None)
def droppixel_reference(case, idx, which, sat=False):
    """-> (map [ndrop, H, W], mask, d z1, d z2 [N, C, H, W]: rows of the images outside idx exactly 0)"""
    o = operands_of(case, sat)
    mask = seeded_mask('drop-%s-%s-%d' % (map_id(case), idx, which), (len(idx), case.h, case.w))
    v, (g1, g2) = masked_backward(lambda a, b: droppixel_map(a, b, o.t, idx, which), (o.z1, o.z2), mask)
    return v, mask, g1, g2


@functools.lru_cache(maxsize=None)
def pixelcoreg_reference(case, three, kd=KD, sat=False):
    """-> (key, val, tf, mask, gradients: (d z3,) with three nets, (d z1, d z2) with two)"""
    o = operands_of(case, sat)
    assert case.c == 2
    mask = seeded_mask('coreg-%s-%d' % (map_id(case), three), o.t.shape)
    if three:
        val, (g3,) = masked_backward(lambda c: pixelcoreg_maps(o.z1.double(), o.z2.double(), c, o.t, kd)[1], (o.z3,), mask)
        key = pixelcoreg_maps(o.z1.double(), o.z2.double(), o.z3.double(), o.t, kd)[0]
        grads = (g3,)
    else:
        key, grads = masked_backward(lambda a, b: pixelcoreg_maps(a, b, None, o.t, kd)[0], (o.z1, o.z2), mask)
        val = key
    return key, val, (o.t != 0).double(), mask, tuple(grads)


# ------------------------------------------------------------------------------------------------- region cross entropy
RegionCase = collections.namedtuple('RegionCase', 'n h w kh kw c')


def region_win(h, w, kh, kw):
    """mirrors `bool region_win` of coteach_ext.hip: the window kernels serve everything but 2x2 windows on even sides"""
    return kh != 2 or kw != 2 or h % 2 != 0 or w % 2 != 0


def grid_blocks(total):
    """mirrors `int grid1`"""
    return max(1, min((total + BLOCK - 1) // BLOCK, GRID_CAP))


def region_count(n, h, w, kh, kw):
    return n * (-(-h // kh)) * (-(-w // kw))


# (N, H, W, KH, KW), every one at C = 2 .. 8.  N = 3: image 2 is all ignored.
REGION_SMALL = (
    (3, 6, 8, 2, 2),        # 2x2 on even sides: the packed-aux kernels (a byte per region at C = 2, a word above)
    (3, 7, 5, 2, 2),        # 2x2 on odd sides: the window kernels, last row and column of windows clipped to 1 pixel
    (3, 10, 10, 3, 3),      # 3x3, the last row / column of windows 1 pixel wide
    (3, 9, 13, 4, 4),       # 4x4, clipped to 1 pixel on both sides
    (3, 5, 7, 1, 3),        # 1xK: single-row windows, last one 1 pixel
    (3, 5, 7, 3, 1),        # Kx1
)
REGION_MULTI_BLOCK = ((3, 46, 50, 2, 2), (3, 46, 50, 3, 3))       # 1725 / 816 regions: 7 / 4 blocks with a ragged tail, C = 2, 5
REGION_LARGE = (
    RegionCase(1, 1026, 1026, 1, 1, 2),     # 1x1: the window kernels past the grid cap (1,052,676 regions)
    RegionCase(1, 2052, 2052, 2, 2, 2),     # the packed two-class kernels past the cap
    RegionCase(1, 2052, 2052, 2, 2, 3),     # the packed C-class kernels past the cap
)
REGION_CASES = tuple(RegionCase(*(g + (c,))) for g in REGION_SMALL for c in CLASS_COUNTS) + \
    tuple(RegionCase(*(g + (c,))) for g in REGION_MULTI_BLOCK for c in (2, 5)) + REGION_LARGE
REGION_SATURATION_CASES = tuple(RegionCase(*(g + (c,))) for g in ((3, 6, 8, 2, 2), (3, 7, 5, 2, 2)) for c in (2, 3, 8))
REGION_ABI_CASES = (RegionCase(3, 46, 50, 2, 2, 2), RegionCase(3, 46, 50, 2, 2, 5), RegionCase(3, 46, 50, 3, 3, 5),
                    RegionCase(3, 7, 5, 2, 2, 4))


def region_id(c):
    return '%dx%dx%d-k%dx%d-c%d' % c


def out_of_class_window(case):
    """the window cases with C >= 3 carry one pooled target that is no class (region 0 of image 1)"""
    return region_win(case.h, case.w, case.kh, case.kw) and case.c >= 3 and case.n > 1


@functools.lru_cache(maxsize=None)
def region_operands(case):
    """-> (z, t).  Image 0: window (0, 0) holds one ignored pixel among labelled ones (the pooled target is a max: the whole
    region is ignored); window (0, 1) is constant in every class plane (every position ties: the first one is the arg-max);
    window (1, 0) holds its maximum at the first and at the last position.  Image 1, the window cases with C >= 3: the
    pooled target of region 0 is C + 1, no class.  Image 2: every pixel ignored."""
    n, h, w, kh, kw, c = case
    g = _seed('region-' + region_id(case))
    z = torch.randn(n, c, h, w, generator=g) * 2
    t = torch.randint(0, c, (n, h, w), generator=g)
    if n > 1:
        t[0, 0, 0] = 1
        t[0, min(kh, h) - 1, min(kw, w) - 1] = IGNORE
        if kh * kw == 1:
            t[0, 0, 0] = IGNORE
        z[0, :, :kh, kw:2 * kw] = torch.arange(1, c + 1, dtype=torch.float32).view(c, 1, 1) * 0.5
        z[0, :, kh:2 * kh, :kw] = z[0, :, kh:2 * kh, :kw].clamp(max=2.5)
        z[0, :, kh, 0] = 3.0
        z[0, :, min(2 * kh, h) - 1, kw - 1] = 3.0
        if out_of_class_window(case):
            t[1, 0, 0] = c + 1
        if n > 2:
            t[2] = IGNORE
    return z, t


def pooled(z, t, kh, kw):
    """MaxPool2d(kernel = stride = (KH, KW), ceil_mode=True) of the logits per class and of the targets as numbers"""
    zp = F.max_pool2d(z, (kh, kw), stride=(kh, kw), ceil_mode=True)
    tp = F.max_pool2d(t.double().unsqueeze(1), (kh, kw), stride=(kh, kw), ceil_mode=True).squeeze(1).long()
    return zp, tp


def region_class(tp, c, win):
    """the class a pooled target stands for, IGNORE where the region does not count.  The packed two-class kernel takes every
    non-zero target as class 1; the C-class and the window kernels ignore a target outside [0, C)"""
    if c == 2 and not win:
        return torch.where(tp == IGNORE, tp, (tp != 0).long())
    return torch.where((tp < 0) | (tp >= c), torch.full_like(tp, IGNORE), tp)


def region_ce(z, t, kh, kw):
    """region cross entropy [N, P] of logits z (any float type) and index targets t"""
    n, c, h, w = z.shape
    zp, tp = pooled(z, t, kh, kw)
    return F.cross_entropy(zp, region_class(tp, c, region_win(h, w, kh, kw)), ignore_index=IGNORE, reduction='none').view(n, -1)


@functools.lru_cache(maxsize=None)
def region_operands_of(case, sat=False):
    """sat: the logits scaled so that differences reach +-80; ties stay ties"""
    z, t = region_operands(case)
    return ((z * (80.0 / (z.max() - z.min()).item())).contiguous() if sat else z), t


@functools.lru_cache(maxsize=None)
def region_reference(case, sat=False):
    """-> (loss [N, P], mask [N, P], dz [N, C, H, W] of COEFF * sum(mask * loss)), float64.  The seeded mask always holds the
    regions the operands were built for: the two tied windows of image 0 (regions 1 and Wp) and region 0 of image 1 (the
    out-of-class pooled target of the window cases), so that their backward is reached whatever the seed"""
    z, t = region_operands_of(case, sat)
    mask = seeded_mask('region-' + region_id(case), (case.n, region_count(1, *case[1:5])))
    if case.n > 1:
        mask[0, 1] = mask[0, -(-case.w // case.kw)] = mask[1, 0] = 1
    v, (dz,) = masked_backward(lambda a: region_ce(a, t, case.kh, case.kw), (z,), mask)
    return v, mask, dz


# ------------------------------------------------------------------------------------------------- k smallest
SelectCase = collections.namedtuple('SelectCase', 'm nseg stride')
SELECT_M = (1, 35, 1023, 1024, 1025, 5000)          # idle threads; cpt 1 | 1 | 2 at 1023 | 1024 | 1025; cpt 5
SELECT_LARGE_M = 1026 * 1026                        # cpt = 1029: the size of the per-pixel selections
SELECT_CASES = tuple(SelectCase(m, nseg, m + pad) for m in SELECT_M for nseg, pad in ((1, 0), (3, 0), (3, 24))) + \
    (SelectCase(SELECT_LARGE_M, 1, SELECT_LARGE_M), SelectCase(SELECT_LARGE_M, 1, SELECT_LARGE_M + 24))
TIE = 0.25


def select_id(c):
    return 'm%d-s%d-stride+%d' % (c.m, c.nseg, c.stride - c.m)


def cpt(m):
    return (m + SELECT_THREADS - 1) // SELECT_THREADS


def tie_run(m):
    """(start, length) of the run of TIE values of segments 0 and 2: longer than cpt, so it crosses thread ranges"""
    length = min(m, 2 * cpt(m) + 3)
    return max(0, m // 2 - length // 2), length


def _specials():
    """+0 before -0 (a key that orders -0 first picks the higher index), both denormals, +inf, NaN of both signs (a key that
    orders a negative NaN first selects it before everything), a negative, -0 before +0"""
    bits = torch.tensor([0x7FC00000, -0x400000], dtype=torch.int32).view(torch.float32)      # +NaN, -NaN (0xFFC00000)
    return torch.cat([torch.tensor([0.0, -0.0, 1e-40, -1e-40, float('inf')]), bits, torch.tensor([-3.5, -0.0, 0.0])])


@functools.lru_cache(maxsize=None)
def select_values(case):
    """-> (sel [nseg, stride] fp32, sum [nseg, stride] fp32 in [0.5, 1.5)); columns past M are NaN and never read.
    Segment 0 and 2: normal draws with negatives, the tie run, and (M >= 35) the special values in slots 0 .. 9;
    segment 1: all equal."""
    m, nseg, stride = case
    g = _seed('select-' + select_id(case))
    sel = torch.full((nseg, stride), float('nan'))
    for s in range(nseg):
        if s == 1:
            sel[s, :m] = 0.5
            continue
        v = torch.randn(m, generator=g)
        a, length = tie_run(m)
        v[a:a + length] = TIE
        if m >= 35:
            v[:10] = _specials()
        sel[s, :m] = v
    return sel, torch.rand(nseg, stride, generator=g) + 0.5


def candidates(v, only_positive):
    return v > 0 if only_positive else torch.ones_like(v, dtype=torch.bool)


def select_ks(case, only_positive):
    """-> list of (k_host, rr, k_in) over the k forms: 0, 1, inside the tie run of segment 0, at the zeros, the candidate
    count less one (NaN sorts last), the count, above it; rr with a non-integral rr * count; k on the device"""
    v = select_values(case)[0][0, :case.m]
    cand = candidates(v, only_positive)
    count = int(cand.sum())
    below = int((cand & (v < TIE)).sum())
    inside = below + (tie_run(case.m)[1] + 1) // 2
    zeros = int((cand & (v < 0)).sum()) + 1
    ks = sorted(set(k for k in (0, 1, inside, zeros, count - 1, count, count + 5) if k >= 0))
    forms = [(k, -1.0, None) for k in ks] + [(0, 0.3703, None), (-1, -1.0, inside)]
    return forms


def select_k(count, k_host, rr, k_in):
    """k as the kernel's header states it, computed as Python computes it"""
    k = k_in if k_in is not None else (int(rr * count) if rr >= 0 else k_host)
    return max(0, min(k, count))


@functools.lru_cache(maxsize=None)
def select_order(case, seg, only_positive):
    """the candidates of a segment in selection order: stable argsort (ties by lower index, +-0 equal, NaN last) of the fp32
    values with the non-candidates removed"""
    v = select_values(case)[0][seg, :case.m]
    idx = candidates(v, only_positive).nonzero().view(-1)
    return idx[torch.sort(v[idx], stable=True).indices]


def select_reference(case, k_host=-1, rr=-1.0, k_in=None, only_positive=False):
    """exact -> (mask [nseg, M] uint8, float64 sums [nseg] of the sum array over the mask, ks [nseg])"""
    m, nseg, _ = case
    sums = select_values(case)[1]
    mask = torch.zeros(nseg, m, dtype=torch.uint8)
    tot, ks = torch.zeros(nseg, dtype=torch.float64), torch.zeros(nseg, dtype=torch.int64)
    for s in range(nseg):
        order = select_order(case, s, only_positive)
        k = select_k(order.numel(), k_host, rr, k_in)
        mask[s, order[:k]] = 1
        tot[s] = sums[s, :m].double()[mask[s].bool()].sum()
        ks[s] = k
    return mask, tot, ks


# ------------------------------------------------------------------------------------------------- the drop-in modules
# The selection values of the k-th and the (k + 1)-th place of every segment are at least 2 * SEL_GAP * max(1, |value|) apart in
# float64 -- an fp32 value carries an error of some 1e-6 of max(1, |value|): a log-sum-exp of logits of size 1 .. 10 less one of
# them -- or both exactly 0.0 (ignored regions: an exact tie in any precision, decided by index).  No rule where k = 0 or k = the
# candidate count: every cut gives the same set.
SEL_GAP = 1e-5
MODULE_GEOMETRY = (3, 46, 50)
REGION_SCALES = (0.5, 0.3, 0.25, 1.0)               # windows 2x2 (packed), 3x3, 4x4, 1x1 on 46 x 50
MODULE_CLASSES = (2, 3, 8)


def cut_gap(values, k, only_positive=False):
    """distance between the k-th and the (k + 1)-th smallest candidate of a float64 vector over max(1, the larger of the two);
    inf where every cut gives the same set or the two are exact zeros"""
    v = values[values > 0] if only_positive else values
    if k <= 0 or k >= v.numel():
        return float('inf')
    s = torch.sort(v).values
    if s[k - 1] == 0 and s[k] == 0:
        return float('inf')
    return ((s[k] - s[k - 1]) / max(1.0, abs(s[k].item()), abs(s[k - 1].item()))).item()


def module_targets(g, n, c, h, w):
    t = torch.randint(0, c, (n, h, w), generator=g)
    t[0, 0, :5] = IGNORE
    return t


def region_windows(h, w, scale):
    return int(h / int(h * scale)), int(w / int(w * scale))


@functools.lru_cache(maxsize=None)
def region_module_operands(c):
    """logits of two nets and targets on MODULE_GEOMETRY whose region losses obey the gap rule at every scale and forget rate"""
    n, h, w = MODULE_GEOMETRY
    for draw in range(32):
        g = _seed('region-module-c%d#%d' % (c, draw))
        z1, z2 = torch.randn(n, c, h, w, generator=g) * 2, torch.randn(n, c, h, w, generator=g) * 2
        t = module_targets(g, n, c, h, w)
        if region_module_gap(z1, z2, t) > 2 * SEL_GAP:
            return z1, z2, t
    raise AssertionError('no draw separates the region losses at the cut, C = %d' % c)


def region_module_gap(z1, z2, t):
    gap = float('inf')
    for scale in REGION_SCALES:
        kh, kw = region_windows(z1.shape[2], z1.shape[3], scale)
        for z in (z1, z2):
            loss = region_ce(z.double(), t, kh, kw)
            for fr in FORGET_RATES:
                keep = int((1 - fr) * loss.shape[1])
                gap = min([gap] + [cut_gap(row, keep) for row in loss])
    return gap


def region_module_reference(z1, z2, t, scale, fr):
    """Coteachingloss_dropregionce: per image the keep regions with the smallest loss of the OTHER net, mean over all kept
    -> dict(loss1, loss2, grad1, grad2, mask1, mask2); mask K selects net K's regions (chosen by the other net's losses)"""
    kh, kw = region_windows(z1.shape[2], z1.shape[3], scale)
    a = [z1.double().requires_grad_(True), z2.double().requires_grad_(True)]
    loss = [region_ce(x, t, kh, kw) for x in a]
    n, p = loss[0].shape
    keep = int((1 - fr) * p)
    out = {}
    for me in (0, 1):
        other = loss[1 - me].detach()
        mask = torch.zeros(n, p, dtype=torch.uint8)
        for i in range(n):
            mask[i, LC.stable_argsort(other[i])[:keep]] = 1
        kept = loss[me][mask.bool()]
        v = kept.sum() / kept.numel() if keep > 0 else kept.sum() * float('nan')      # the mean of an empty set is NaN ...
        g, = torch.autograd.grad(v, a[me])                                            # ... and its gradient 0
        out['loss%d' % (me + 1)], out['grad%d' % (me + 1)], out['mask%d' % (me + 1)] = v.detach(), g, mask
    return out


@functools.lru_cache(maxsize=None)
def pixel_module_operands(c):
    """LC.coteach_operands (per-image losses apart: the image ranking is exact) drawn again until the pixel selections of
    Coteachingloss_dropimagedroppixel and, for two classes, of both Pixelcoreg_Focalloss* obey the gap rule too.
    -> (z1, z2, z3, t)"""
    n = MODULE_GEOMETRY[0]
    o = LC.coteach_operands(n, c)
    h, w = LC.COTEACH_HW
    for draw in range(32):
        g = _seed('pixel-module-c%d#%d' % (c, draw))
        z3 = torch.randn(n, c, h, w, generator=g) * 2
        z2 = (o.z2 + torch.randn(n, c, h, w, generator=g) * (1e-3 * draw)).contiguous()
        # two classes: no ignored pixel, where the two-class drop-pixel kernel (every non-zero target is class 1) and the
        # reference (no CE term there) part ways; the map-level cases hold the kernel to its own rule
        t = LC.index_targets(o.t1) if c == 2 else o.t1
        if pixel_module_gap(o.z1, z2, z3, t) > 2 * SEL_GAP and \
                LC.coteach_min_gap(o._replace(z2=z2, t1=t, t2=t)) > 2 * LC.MIN_GAP:
            return o.z1, z2, z3, t
    raise AssertionError('no draw separates the pixel values at the cut, C = %d' % c)


def droppixel_keep(fr, n):
    return int((1 - fr) * n)


def pixel_module_gap(z1, z2, z3, t):
    n, c = z1.shape[:2]
    gap = float('inf')
    a, b = z1.double(), z2.double()
    for fr in FORGET_RATES:
        keep = droppixel_keep(fr, n)
        if 0 < keep < n:
            r = LC.coteach_reference(z1, z2, t, t, 1, keep, 1.0, 1.0)
            d1, d2 = r['argsort1'][keep:], r['argsort2'][keep:]
            v1 = droppixel_map(a, b, t, d2, 0).view(-1)
            k2 = int((1 - fr) * int((v1 > 0).sum()))
            gap = min(gap, cut_gap(v1, k2, True), cut_gap(droppixel_map(a, b, t, d1, 1).view(-1), k2, True))
        if c == 2:
            hw = z1.shape[2] * z1.shape[3]
            for zz in (z3.double(), None):
                for kd in (0.3, 0.7):
                    key = pixelcoreg_maps(a, b, zz, t, kd)[0].view(n, -1)
                    gap = min([gap] + [cut_gap(row, int((1 - fr) * hw)) for row in key])
    return gap


def droppixel_module_reference(z1, z2, t, fr, weight=1.0):
    """Coteachingloss_dropimagedroppixel: the image-level dropimage losses plus 0.25 x the mean of the keep2 smallest positive
    values of the drop-pixel map on the images the OTHER net's ranking drops; branch 2 keeps as many pixels as branch 1.
    A dropped set without a positive value gives NaN (the mean of an empty set), as in the reference.
    -> dict(loss1, loss2, l1_grad1, l1_grad2, l2_grad1, l2_grad2, mask1, mask2 (None without a pixel term), count1, count2)"""
    n = z1.shape[0]
    keep = droppixel_keep(fr, n)
    base = LC.coteach_reference(z1, z2, t, t, 1, keep, weight, 1.0)
    out = dict(loss1=base['loss1'], loss2=base['loss2'], l1_grad1=base['grad1'], l1_grad2=torch.zeros_like(base['grad2']),
               l2_grad1=torch.zeros_like(base['grad1']), l2_grad2=base['grad2'], mask1=None, mask2=None)
    if keep >= n:
        return out
    d1, d2 = base['argsort1'][keep:], base['argsort2'][keep:]
    k2 = None
    for me, idx in ((0, d2), (1, d1)):
        a, b = z1.double().requires_grad_(True), z2.double().requires_grad_(True)
        v = droppixel_map(a, b, t, idx, me).view(-1)
        cand = (v.detach() > 0).nonzero().view(-1)
        if k2 is None:
            k2 = int((1 - fr) * cand.numel())
        k = min(k2, cand.numel())
        sel = cand[LC.stable_argsort(v.detach()[cand])[:k]]
        term = v[sel].sum() / k if k > 0 else v[sel].sum() * float('nan')
        ga, gb = torch.autograd.grad(0.25 * term, (a, b))
        mask = torch.zeros(v.numel(), dtype=torch.uint8)
        mask[sel] = 1
        tag = 'l%d' % (me + 1)
        out['loss%d' % (me + 1)] = out['loss%d' % (me + 1)] + 0.25 * term.detach()
        out[tag + '_grad1'], out[tag + '_grad2'] = out[tag + '_grad1'] + ga, out[tag + '_grad2'] + gb
        out['mask%d' % (me + 1)] = mask
        out['count%d' % (me + 1)] = cand.numel()
    return out


def pixelcoreg_module_reference(z1, z2, z3, t, fr, kd, reduction):
    """Pixelcoreg_Focalloss (z3 given) / _twomodel (z3 None): per image the int((1 - fr) HW) pixels with the smallest key; the
    mean or sum of val over all kept; the kept share of the foreground -> dict(loss, frac, grads, mask)"""
    n, hw = z1.shape[0], z1.shape[2] * z1.shape[3]
    leaves = [x.double().requires_grad_(True) for x in ((z1, z2, z3) if z3 is not None else (z1, z2))]
    key, val, tf = pixelcoreg_maps(leaves[0], leaves[1], leaves[2] if z3 is not None else None, t, kd)
    keep = int((1 - fr) * hw)
    mask = torch.zeros(n, hw, dtype=torch.uint8)
    for i in range(n):
        mask[i, LC.stable_argsort(key.detach().view(n, -1)[i])[:keep]] = 1
    kept = val.view(n, -1)[mask.bool()]
    if reduction == 'mean':
        loss = kept.sum() / kept.numel() if keep > 0 else kept.sum() * float('nan')
    else:
        loss = kept.sum()
    wrt = leaves[2:] if z3 is not None else leaves
    grads = list(torch.autograd.grad(loss, wrt))
    frac = tf.view(n, -1)[mask.bool()].sum() / tf.sum()
    return dict(loss=loss.detach(), frac=frac, grads=grads, mask=mask)


def structural_zeros_hold(got, ref):
    """wherever the float64 gradient is exactly 0.0 (outside the mask, ignored, not the arg-max, another image) the kernel's
    is exactly 0.0 too"""
    got = got.detach().cpu()
    return bool((got.reshape(ref.shape)[ref == 0] == 0).all())
