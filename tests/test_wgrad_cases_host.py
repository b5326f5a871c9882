"""CPU: makes the case table of tests/wgrad_cases.py binding.  Host-side queries of the library only (split counts and
`supported`), the slab reduce's group rule mirrored below, and plain torch: every case is accepted by its family, every
branch test_gpu_wgrad_slabs.py is meant to reach has a case that reaches it (an assert, not a skip), the float64 reference
agrees with autograd, and every case is small and rough enough for one missing dz pixel to show far above its tolerance.
Run with -s for the table of split and group counts the library reports."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as WC


@pytest.fixture(scope='module')
def L():
    from aide_amd.build import build
    build(verbose=False)
    from aide_amd._lib import lib
    return lib.load()            # raw entry points: host-state queries


def reduce_groups(splits, cc):
    # mirrors reduce_groups() in aide_amd/csrc/conv3x3_wgrad.hip (split groups per workgroup of the 16-byte slab reduce; a
    # workgroup covers R = 1024 / groups (co, ci) pairs).  When that rule changes this test fails and the table is re-picked.
    return 16 if splits >= 16 else 4 if splits >= 4 else 4 if splits >= 2 and cc <= 256 * 256 else 1


def splits_of(L, c):
    dims = (c.n, c.co, c.ci, c.h, c.w)
    if c.family in ('direct', 'stem'):
        return L.aide_conv3x3_wgrad_splits(*dims)
    if c.family == 'wino2':
        return L.aide_conv3x3_wgrad_wino_splits(*dims)
    if c.family == 'wino4':
        return L.aide_conv3x3_wgrad_wino4_splits_t(*(dims + (c.target_wgs,)))
    return L.aide_conv3x3_wgrad_bf16_splits(*(dims + (c.co_blocks,)))


def direct_variant(co, ci):
    """wgrad_variant() of conv3x3_wgrad.hip: 0 = 64 co x 64 ci, 1 = 32 x 64, 2 = 64 x 32, 3 = 32 x 32"""
    return 0 if co >= 64 and ci >= 64 else 1 if ci >= 64 else 2 if co >= 64 else 3


def ragged(c):
    return c.h % 4 != 0 or c.w % 16 != 0


def units_per_image(c):
    """work units (tiles or chunks) of one image, as each kernel cuts it"""
    cdiv = lambda a, b: (a + b - 1) // b
    return {'direct': cdiv(c.h, 4) * cdiv(c.w, 16), 'stem': (c.h // 4) * (c.w // 64), 'stem_bf16': (c.h // 4) * (c.w // 64),
            'wino2': (c.h // 2) * cdiv(c.w, 16), 'wino4': (c.h // 4) * cdiv(c.w, 16), 'bf16': (c.h // 4) * (c.w // 32)}[c.family]


def split_crosses_images(c, splits):
    """N >= 2, the units do not divide by the split count, and one split's units lie in two images.  The stem kernel deals
    its tiles round-robin (tile = split, split + splits, ...), the others give a split one contiguous range."""
    upi = units_per_image(c)
    units = c.n * upi
    if c.n < 2 or units % splits == 0:
        return False
    if c.family in ('stem', 'stem_bf16'):
        ranges = [list(range(s, units, splits)) for s in range(min(splits, units))]
    else:
        per = (units + splits - 1) // splits
        ranges = [list(range(s * per, min((s + 1) * per, units))) for s in range(splits)]
    return any(len(r) >= 2 and r[0] // upi != r[-1] // upi for r in ranges)


@pytest.fixture(scope='module')
def rows(L):
    """[(case, splits, groups, cc)] and, with -s, the table"""
    out = []
    print()
    for c in WC.CASES:
        s = splits_of(L, c)
        cc = c.co * c.ci
        g = reduce_groups(s, cc)
        out.append((c, s, g, cc))
        print('%-44s splits %3d  groups %2d  pairs %6d = %7.3f workgroups of %4d   units %3d%s' % (
            WC.case_id(c), s, g, cc, cc / (1024.0 / g), 1024 // g, c.n * units_per_image(c),
            '  (scalar reduce)' if cc % 4 else ''))
    return out


def test_table_is_well_formed():
    assert len(set(WC.CASES)) == len(WC.CASES) and len(set(map(WC.case_id, WC.CASES))) == len(WC.CASES)
    for c in WC.CASES:
        assert c.family in WC.FAMILIES and c.family in WC.TOL
        assert c.store in ('fp32', 'bf16', 'dz_bf16') and (c.store == 'fp32' or WC.bf16_contract(c)), c
        assert c.store != 'bf16' or c.family == 'bf16', c          # the stem kernel reads the fp32 image
        assert (c.target_wgs == 0 or c.family == 'wino4') and (c.co_blocks == 0 or c.family == 'bf16'), c
    for f in WC.FAMILIES:
        assert any(c.family == f and c.misaligned for c in WC.CASES), 'no misaligned-dw case for %s' % f


def test_every_case_is_supported_by_its_family(L):
    for c in WC.CASES:
        shape = (c.co, c.ci, c.h, c.w)
        stem = L.aide_conv3x3_wgrad_stem_supported(*shape)
        if c.family == 'direct':
            assert not stem, c                 # aide_conv3x3_wgrad would hand it to the stem kernel
        elif c.family == 'stem':
            assert stem, c
        elif c.family == 'stem_bf16':
            assert stem and L.aide_conv3x3_wgrad_bf16_supported(*shape), c
        elif c.family == 'bf16':
            assert L.aide_conv3x3_wgrad_bf16_supported(*shape) and not stem, c
        elif c.family == 'wino2':
            assert L.aide_conv3x3_wgrad_wino_supported(*shape), c
        else:
            assert L.aide_conv3x3_wgrad_wino4_supported(*shape), c


def test_required_branches_are_reached(rows):
    def need(what, pred):
        hit = [WC.case_id(c) for c, s, g, cc in rows if pred(c, s, g, cc)]
        assert hit, 'no case reaches: ' + what
    for groups in (1, 4, 16):
        r = 1024 // groups
        need('%d groups, Co*Ci > R = %d with a partial last workgroup' % (groups, r),
             lambda c, s, g, cc: g == groups and cc % 4 == 0 and cc > r and cc % r != 0)
        need('%d groups, Co*Ci < R = %d' % (groups, r), lambda c, s, g, cc: g == groups and cc % 4 == 0 and cc < r)
    need('splits == 1', lambda c, s, g, cc: s == 1)
    need('2 or 3 splits with Co*Ci > 65536', lambda c, s, g, cc: s in (2, 3) and cc > 65536 and cc % 4 == 0 and g == 1)
    need('Co*Ci % 4 != 0', lambda c, s, g, cc: cc % 4 != 0)
    for v in range(4):
        for rg in (True, False):
            need('direct variant %d, %s' % (v, 'ragged' if rg else 'dense'),
                 lambda c, s, g, cc: c.family == 'direct' and direct_variant(c.co, c.ci) == v and ragged(c) == rg)
    need('stem kernel, fp32 entry', lambda c, s, g, cc: c.family == 'stem')
    need('stem kernel, bf16 entry', lambda c, s, g, cc: c.family == 'stem_bf16')
    need('stem kernel, bf16 entry, bf16-stored dz', lambda c, s, g, cc: c.family == 'stem_bf16' and c.store == 'dz_bf16')
    need('F(2x2)', lambda c, s, g, cc: c.family == 'wino2')
    need('F(4x4), default target', lambda c, s, g, cc: c.family == 'wino4' and c.target_wgs == 0)
    need('F(4x4), explicit target', lambda c, s, g, cc: c.family == 'wino4' and c.target_wgs > 0)
    need('F(4x4), trailing half co tile', lambda c, s, g, cc: c.family == 'wino4' and c.co % 64 == 32)
    for cb in (1, 2, 4):                       # (4 co blocks need Co % 128 == 0: wgrad_bf16_nwco, conv3x3_bf16.hip)
        need('bf16 kernel, co_blocks %d' % cb,
             lambda c, s, g, cc: c.family == 'bf16' and c.co_blocks == cb and (cb != 4 or c.co % 128 == 0))
    need('bf16 kernel, bf16-stored operands', lambda c, s, g, cc: c.family == 'bf16' and c.store == 'bf16')
    for f in WC.FAMILIES:
        need('%s: N >= 2 and a split that crosses an image boundary' % f,
             lambda c, s, g, cc: c.family == f and split_crosses_images(c, s))


def test_explicit_f4_targets_change_the_split_count(L, rows):
    for c, s, g, cc in rows:
        if c.family == 'wino4' and c.target_wgs:
            assert s != L.aide_conv3x3_wgrad_wino4_splits(c.n, c.co, c.ci, c.h, c.w), c


def test_batch_boundary_case_is_the_smallest_summing_one(rows):
    c, s, g, cc = [r for r in rows if r[0] == WC.BOUNDARY_CASE][0]
    assert s == 2 and cc % 4 == 0 and c.n * c.h * c.w == 128


SMALL = [c for c in WC.CASES if c.n * c.h * c.w * c.co * c.ci <= 1 << 20][:3]


@pytest.mark.parametrize('c', SMALL, ids=WC.case_id)
def test_reference_is_the_autograd_of_conv2d(c):
    x, dz = WC.operands(c)
    w = torch.zeros(c.co, c.ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, padding=1).backward(dz.double())
    assert len(SMALL) == 3 and WC.rel_err(WC.reference_dw(x, dz), w.grad) <= 1e-12


@pytest.mark.parametrize('c', WC.CASES, ids=WC.case_id)
def test_one_missing_pixel_shows(c):
    """the last pixel of the last row of the last image, where ragged tiles end: without it the reference moves by more than
    ten times the tolerance the case is held to"""
    x, dz = WC.operands(c)
    dz0 = dz.clone()
    dz0[-1, :, -1, -1] = 0.0
    ref = WC.reference(c)
    moved = WC.rel_err(WC.reference_dw(*WC.contract_operands(c, x, dz0)), ref)
    assert moved > 10 * WC.TOL[c.family], '%s: %.3e' % (WC.case_id(c), moved)


def test_bf16_contract_rounds_the_operands():
    c = [c for c in WC.CASES if c.family == 'bf16' and c.store == 'fp32'][0]
    x, dz = WC.operands(c)
    assert WC.rel_err(WC.reference_dw(x, dz), WC.reference(c)) > 10 * WC.TOL['bf16']      # the rounding is not a no-op
    c = [c for c in WC.CASES if c.store == 'bf16'][0]
    x, dz = WC.operands(c)
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dz.bfloat16().float(), dz)


def test_guard_helpers():
    dev = torch.device('cpu')
    for lead in (WC.LEAD, WC.LEAD_MISALIGNED):
        buf, view = WC.guarded(10, lead, dev)
        assert buf.numel() == lead + 10 + 4096 and view.numel() == 10 and view.data_ptr() == buf.data_ptr() + 4 * lead
        assert (view.data_ptr() % 16 == 0) == (lead == WC.LEAD)
        assert bool(torch.isnan(buf).all()) and WC.all_pattern(view) and WC.guards_intact(buf, lead, 10)
        view.fill_(1.0)
        assert WC.guards_intact(buf, lead, 10) and not WC.all_pattern(view)
        for i in (0, lead - 1, lead + 10, buf.numel() - 1):
            b2 = buf.clone()
            b2[i] = float('nan')                 # another NaN: the comparison is on the bits
            assert not WC.guards_intact(b2, lead, 10), i
