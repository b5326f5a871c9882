"""-m gpu: the pieces that the three pseudo-label banks share on the device (aide_amd/csrc/labelbank.hip): one ranking kernel
behind `aide_label_refresh_select`, `aide_label_refresh_select_classes` and `aide_image_refresh_select`, one rewrite kernel
behind `aide_label_bank_update`, `aide_label_bank_update_classes` and `aide_image_bank_update`.  Every result is compared
with its host rule / numpy and with the other entry points on inputs where the definitions coincide.  Exact: no tolerance."""
import numpy as np
import pytest
import torch

import refresh_shared_cases as rc

pytestmark = pytest.mark.gpu


def _select(form, sums, labelled, n_select, dev):
    """-> (dice, rank, flag) as numpy from the entry point of `form` ('binary', 'classes': the C = 2 counts, 'image')"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    k = len(sums)
    dice = torch.full((k,), -7.0, device=dev, dtype=torch.float32)
    rank = torch.full((k,), -7, device=dev, dtype=torch.int32)
    flag = torch.full((k,), 7, device=dev, dtype=torch.uint8)
    lab = torch.from_numpy(labelled).to(dev) if labelled is not None else None
    out = (ptr(dice), ptr(rank), ptr(flag), stream_ptr())
    if form == 'classes':
        counts = torch.from_numpy(rc.counts_c2(sums)).to(dev)
        cd = torch.empty(k, 2, device=dev, dtype=torch.float32)
        check(lib.aide_label_refresh_select_classes(ptr(counts), ptr(lab), k, 2, n_select, ptr(cd), *out), 'select_classes')
    else:
        s = torch.from_numpy(sums).to(dev)
        fn = lib.aide_label_refresh_select if form == 'binary' else lib.aide_image_refresh_select
        check(fn(ptr(s), ptr(lab), k, n_select, *out), 'select ' + form)
    return tuple(x.cpu().numpy() for x in (dice, rank, flag))


@pytest.mark.parametrize('K', [1, 1023, 1024, 1025, 4096])
def test_one_ranking_behind_three_entry_points(dev, K):
    """A workgroup of the ranking kernel owns 1024 items: 1023 and 1025 put the last item on either side of that edge, 4096 is
    the case forms' limit and fills one LDS tile of keys."""
    from aide_amd.inference import case_dice_rule, case_dice_rule_classes, image_dice_rule
    sums, labelled, n = rc.shared_sums(K, K)
    for lab, n_select in ((labelled, n), (None, n), (labelled, K + 3)):
        want = case_dice_rule(sums, lab, n_select)
        assert all(rc.same_bits(a, b) for a, b in zip(want, case_dice_rule_classes(rc.counts_c2(sums), lab, n_select)[1:]))
        assert all(rc.same_bits(a, b) for a, b in zip(want, image_dice_rule(sums, lab, n_select)))
        for form in ('binary', 'classes', 'image'):
            got = _select(form, sums, lab, n_select, dev)
            for name, a, b in zip(('dice', 'rank', 'flag'), got, want):
                assert rc.same_bits(a, b), (K, form, n_select, name)
    if K > 1:
        assert rc.boundary_tie(want[0], want[1], n) and labelled.any()
    if K >= 8:                                   # rows with sum p + sum t = 0: NaN in the case forms, 0.0 in the image form
        sums, labelled, n = rc.shared_sums(K + 1, K, zero_rows=True)
        want = case_dice_rule(sums, labelled, n)
        assert np.isnan(want[0]).sum() == K // 8 and rc.boundary_tie(want[0], want[1], n)
        for form in ('binary', 'classes'):
            for name, a, b in zip(('dice', 'rank', 'flag'), _select(form, sums, labelled, n, dev), want):
                assert rc.same_bits(a, b), (K, form, 'empty rows', name)
        for name, a, b in zip(('dice', 'rank', 'flag'), _select('image', sums, labelled, n, dev), image_dice_rule(sums, labelled, n)):
            assert rc.same_bits(a, b), (K, 'image', 'empty rows', name)


def _place(x, dev, odd):
    """the bytes of x on the device, at an odd address if asked"""
    if not odd:
        return torch.from_numpy(x).to(dev)
    flat = torch.zeros(x.size + 1, dtype=torch.uint8, device=dev)
    flat[1:].copy_(torch.from_numpy(x).reshape(-1))
    v = flat[1:].view(x.shape)
    assert v.data_ptr() % 2 == 1 and v.is_contiguous()
    return v


def _update(form, pred, flags, st, scale, bank, dev, odd):
    """-> the whole plane after the update entry point of `form` ('scale', 'palette': (0, scale) with C = 2, 'image')"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    pred_d, bank_d = torch.from_numpy(pred).to(dev), _place(bank, dev, odd)
    flag_d = torch.from_numpy(flags).to(dev)
    st_d = torch.from_numpy(st).to(dev)
    k = len(flags)
    if form == 'image':
        assert pred.shape[0] == k
        check(lib.aide_image_bank_update(ptr(pred_d), ptr(flag_d), *pred.shape, scale, ptr(bank_d), stream_ptr()), 'image_bank_update')
    elif form == 'palette':
        pal = torch.tensor([0, scale], dtype=torch.int32, device=dev)
        check(lib.aide_label_bank_update_classes(ptr(pred_d), ptr(flag_d), ptr(st_d), k, *pred.shape, ptr(pal), 2, ptr(bank_d),
                                                 stream_ptr()), 'label_bank_update_classes')
    else:
        check(lib.aide_label_bank_update(ptr(pred_d), ptr(flag_d), ptr(st_d), k, *pred.shape, scale, ptr(bank_d), stream_ptr()),
              'label_bank_update')
    return bank_d.cpu().numpy()


K_UPDATE = 9
FLAGS = {'none': np.zeros(K_UPDATE, np.uint8), 'all': np.ones(K_UPDATE, np.uint8),
         'alternating': (np.arange(K_UPDATE) % 2).astype(np.uint8), 'alternating, even': (np.arange(K_UPDATE) % 2 == 0).astype(np.uint8)}
PLANES = [((5, 7), False), ((16, 16), False), ((16, 16), True)]      # scalar path, vector path, scalar path on a 16-byte plane


@pytest.mark.parametrize('scale', [63, 255])
def test_one_rewrite_behind_three_entry_points(dev, scale):
    """Whole planes against numpy, so the bytes of an unflagged neighbour are checked too.

    The launcher gives a case `chunks = min(4 * ceil(hw / per), 1024)` workgroups, per = 4096 bytes (vector path) or 256
    (scalar path), and a workgroup walks its case in steps of chunks * 256 threads * 16 bytes or 1 byte.  At 16x16 that is 4
    workgroups and 16384 bytes a step on the vector path, 4 workgroups and 1024 bytes a step on the scalar path (odd address);
    at 5x7 4 workgroups and 1024 bytes.  The long case of the ragged table has 70 slices: 17920 bytes at 16x16, so the first
    workgroups go through the loop twice on the vector path and 18 times on the scalar path, and 2450 bytes at 5x7, three
    times.  The image form has one workgroup per 4096 bytes of a plane, a single step at these sizes."""
    rng = np.random.RandomState(scale)
    ragged = np.array([2, 1, 3, 0, 70, 1, 2, 4, 1])                 # an empty case in the middle, a long one after it
    assert len(ragged) == K_UPDATE
    for (h, w), odd in PLANES:
        # uniform planes: the table arange(K + 1) against the image form, on a map of every byte value
        pred = rng.randint(0, 256, (K_UPDATE, h, w)).astype(np.uint8)
        pred01 = (pred & 1).astype(np.uint8)
        bank = rng.randint(0, 256, pred.shape).astype(np.uint8)
        st = np.arange(K_UPDATE + 1, dtype=np.int64)
        for name, flags in FLAGS.items():
            want = np.where(flags.astype(bool)[:, None, None], (pred.astype(np.int64) * scale).astype(np.uint8), bank)
            for form in ('scale', 'image'):
                assert np.array_equal(_update(form, pred, flags, st, scale, bank, dev, odd), want), (form, h, w, odd, name)
            want = np.where(flags.astype(bool)[:, None, None], pred01 * np.uint8(scale), bank)
            for form in ('scale', 'palette', 'image'):
                assert np.array_equal(_update(form, pred01, flags, st, scale, bank, dev, odd), want), (form, h, w, odd, name)
        # the ragged table: the scale map against the palette (0, scale) on a {0, 1} map
        st = np.concatenate([[0], np.cumsum(ragged)]).astype(np.int64)
        pred01 = rng.randint(0, 2, (int(st[-1]), h, w)).astype(np.uint8)
        bank = rng.randint(0, 256, pred01.shape).astype(np.uint8)
        for name, flags in FLAGS.items():
            want = bank.copy()
            for k in np.flatnonzero(flags):
                want[st[k]:st[k + 1]] = pred01[st[k]:st[k + 1]] * np.uint8(scale)
            for form in ('scale', 'palette'):
                assert np.array_equal(_update(form, pred01, flags, st, scale, bank, dev, odd), want), (form, h, w, odd, name)
