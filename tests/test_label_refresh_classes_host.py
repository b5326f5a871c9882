"""The per-class (multi-organ) pseudo-label refresh on the host: `case_class_counts` and `case_dice_rule_classes` of
aide_amd/inference.py are the definition the device path is held to (the reference refreshes the liver only), the numpy
`PseudoLabelBank(num_classes=C)` applies them, and with C = 2 everything is the binary refresh bit for bit.  Integers, bytes
and single fp64 operations only: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import label_refresh_classes_cases as lc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_label_refresh.npz')


@pytest.mark.parametrize('C', [2, 3, 5, 8])
def test_counts_equal_the_plain_loop(C):
    from aide_amd.inference import case_class_counts
    pal = lc.PALETTES[C]
    for ns, (h, w) in ((lc.RAGGED, (5, 7)), ([3], (16, 16)), ([0, 2], (4, 4))):
        lab, bank, st = lc.random_maps(C, ns, h, w, pal)
        got = case_class_counts(lab, bank, st, pal)
        assert got.dtype == np.int64 and got.shape == (len(ns), C, 3)
        assert np.array_equal(got, lc.loop_counts(lab, bank, st, pal))
        if h == 5:
            assert (lab >= C).any() and not np.isin(bank, pal).all()  # values >= C and off-palette bytes are present
        assert np.array_equal(case_class_counts(lab.astype(np.int64), bank, st.tolist(), list(pal)), got)
    assert not got[0].any() and got[1].any()                          # the empty case's rows are zero


def test_counts_reject_a_bad_palette():
    from aide_amd.inference import case_class_counts
    z = np.zeros((1, 2, 2), np.uint8)
    for pal in ((0, 63, 63), (0, 256), (0, -1)):
        with pytest.raises(ValueError):
            case_class_counts(z, z, [0, 1], pal)


def test_score_rule_by_hand():
    from aide_amd.inference import case_dice_rule_classes
    # rows (I, P, T) of background, organ 1, organ 2, organ 3
    counts = np.array([
        [[9, 9, 9], [2, 4, 4], [0, 0, 0], [3, 3, 5]],      # organ 2 absent on both sides: mean of 0.5 and 0.75
        [[9, 9, 9], [2, 4, 4], [0, 5, 0], [3, 3, 5]],      # organ 2 only predicted: scores 0, mean of three
        [[9, 9, 9], [0, 0, 0], [0, 0, 0], [0, 0, 0]],      # no organ at all: NaN, ranks last
        [[0, 0, 0], [5, 10, 10], [0, 0, 0], [6, 8, 8]],    # 0.5 and 0.75 again: equal to case 0, the lower index first
        [[9, 9, 9], [0, 0, 3], [0, 0, 0], [0, 0, 0]],      # organ 1 only in the pseudo-label: 0
        [[9, 9, 9], [4, 4, 4], [1, 1, 1], [2, 2, 2]],      # 1.0
    ], np.int64)
    cd, dice, rank, sel = case_dice_rule_classes(counts, labelled=[0, 0, 0, 0, 1, 0], n_select=3)
    assert cd.dtype == np.float32 and cd.shape == (6, 4) and dice.dtype == np.float32
    assert rank.dtype == np.int32 and sel.dtype == np.uint8
    with np.errstate(invalid='ignore'):
        nan = np.float64(0) / np.float64(0)                # the NaN of the division, as in the binary rule
    want = np.array([0.625, (0.5 + 0.0 + 0.75) / 3.0, nan, 0.625, 0.0, 1.0], np.float64).astype(np.float32)
    assert lc.same_bits(dice, want)
    assert np.isnan(cd[0, 2]) and cd[0, 0] == 1.0 and np.isnan(cd[3, 0]) and cd[1, 2] == 0.0 and cd[3, 3] == 0.75
    assert rank.tolist() == [2, 1, 5, 3, 0, 4]
    assert sel.tolist() == [1, 1, 0, 0, 0, 0]              # case 4 is labelled: ranked first, never selected, slot not handed on
    assert case_dice_rule_classes(counts, n_select=0)[3].tolist() == [0] * 6
    for n in (6, 7, 100):
        assert case_dice_rule_classes(counts, n_select=n)[3].tolist() == [1] * 6
        assert case_dice_rule_classes(counts, [0, 0, 0, 0, 1, 0], n)[3].tolist() == [1, 1, 1, 1, 0, 1]


def test_score_is_one_rounding_of_the_float64_mean():
    from aide_amd.inference import case_dice_rule_classes
    counts = np.zeros((1, 4, 3), np.int64)
    counts[0, 1] = [1, 1, 2]                               # 2/3
    counts[0, 2] = [16777217, 16777217, 50331653]
    counts[0, 3] = [1, 3, 4]                               # 2/7
    d = [np.float64(2 * i) / np.float64(p + t) for i, p, t in counts[0, 1:]]
    want = np.float32(((d[0] + d[1]) + d[2]) / np.float64(3))
    cd, dice, _, _ = case_dice_rule_classes(counts)
    assert dice.view(np.uint32)[0] == want.view(np.uint32)
    assert lc.same_bits(cd[0, 1:], np.asarray(d).astype(np.float32))


def _binary_vs_two_classes(lab, st, plane, labelled, n_select, keep_largest):
    from aide_amd.inference import evaluate_label_maps
    a = evaluate_label_maps(lab, st, plane, 63, labelled, n_select, keep_largest)
    b = evaluate_label_maps(lab, st, plane, labelled=labelled, n_select=n_select, keep_largest=keep_largest, num_classes=2,
                            palette=(0, 63))
    assert sorted(b) == ['class_dice', 'counts', 'dice', 'filtered', 'rank', 'selected']
    for key in ('dice', 'rank', 'selected', 'filtered'):
        assert lc.same_bits(a[key], b[key]), key
    assert np.array_equal(a['sums'][:, 1:], b['counts'][:, 1])
    return a


def test_two_classes_are_the_binary_refresh():
    from aide_amd.labelbank import PseudoLabelBank
    from aide_amd.synthetic import chaos_cases
    cs = chaos_cases(8, 32, seed=11, slices=(1, 5), labelled=(0, 5))
    st = cs['slice_start']
    rng = np.random.RandomState(2)
    truth = (cs['truth'].numpy() == 63).astype(np.int64)
    maps = [np.roll(truth, (1 + n, 2), (1, 2)) | (rng.rand(*truth.shape) < 0.03) for n in range(4)]
    lab8 = np.zeros(8, np.uint8)
    lab8[[0, 5]] = 1
    for m in maps[:2]:
        r = _binary_vs_two_classes(m, st, cs['initial'].numpy(), lab8, 2, True)
        assert np.isfinite(r['dice']).any()
    banks = [PseudoLabelBank(cs['initial'].numpy(), st, cs['labelled'], palette=(0, 63), **kw) for kw in ({}, {'num_classes': 2})]
    for bank in banks:
        assert bank.refresh_from_labels(maps[0], maps[1], 0, 1)
        assert not bank.refresh_from_labels(maps[2], maps[3], 1, 1)
    assert np.array_equal(banks[0].bank, banks[1].bank) and not np.array_equal(banks[0].bank[0], cs['initial'].numpy())
    assert lc.same_bits(banks[0].case_dice().numpy(), banks[1].case_dice().numpy())
    assert np.array_equal(banks[0].rank, banks[1].rank) and np.array_equal(banks[0].modified, banks[1].modified)
    # g23's label maps against its initial masks (five palette bytes; with the palette (0, 63) the others are in no class)
    g = np.load(GOLD)
    for key in ('k9', 'k3'):
        st = g[key + '/slice_start'].tolist()
        lab = np.zeros(len(st) - 1, np.uint8)
        lab[g[key + '/labelled']] = 1
        for n in (1, 2):
            _binary_vs_two_classes(g['%s/e0/gen%d' % (key, n)], st, g[key + '/init'], lab, int(0.25 * len(lab)), False)


def test_numpy_bank_five_classes():
    from aide_amd.labelbank import PseudoLabelBank, CHAOS_PALETTE
    from aide_amd.synthetic import chaos_cases_multiorgan
    from aide_amd.inference import evaluate_label_maps
    C = 5
    cs = chaos_cases_multiorgan(8, C, 32, seed=5, slices=(2, 5), labelled=(0, 3))
    st = cs['slice_start']
    init = cs['initial'].numpy()
    assert set(np.unique(cs['truth'].numpy())) <= set(CHAOS_PALETTE) and len(np.unique(cs['truth'].numpy())) == C
    m1, m2 = lc.class_maps(cs, C, seed=1)
    bank = PseudoLabelBank(init, st, cs['labelled'], num_classes=C)
    assert bank.n_select == 2
    want = []
    for n, m in enumerate((m1, m2)):
        r = evaluate_label_maps(m, st, init, labelled=bank.labelled_host, n_select=2, num_classes=C, palette=CHAOS_PALETTE)
        assert set(np.unique(r['filtered'])) <= set(range(C))
        w = init.copy()
        for k in np.flatnonzero(r['selected']):
            w[st[k]:st[k + 1]] = np.asarray(CHAOS_PALETTE, np.uint8)[r['filtered'][st[k]:st[k + 1]]]
        want.append((r, w))
    assert bank.refresh_from_labels(m1, m2, 0, 1)          # the gate is open
    for n, (r, w) in enumerate(want):
        sel = np.flatnonzero(r['selected'])
        assert len(sel) >= 1 and not set(sel.tolist()) & {0, 3}
        assert np.array_equal(bank.bank[n], w) and not np.array_equal(w, init)
        for k in range(8):                                 # exactly the selected cases changed
            assert (k in sel) or np.array_equal(bank.bank[n, st[k]:st[k + 1]], init[st[k]:st[k + 1]])
        assert np.array_equal(bank.selected[n], r['selected']) and np.array_equal(bank.modified[n], r['selected'])
        assert lc.same_bits(bank.case_dice().numpy()[n], r['dice'])
        assert lc.same_bits(bank.class_dice().numpy()[n], r['class_dice'])
    assert tuple(bank.class_dice().shape) == (2, 8, C) and bank.class_dice().dtype == torch.float32
    held = bank.bank.copy()
    assert not bank.refresh_from_labels(m2, m1, 1, 1)      # the gate is closed: scored, ranked, nothing written
    assert np.array_equal(bank.bank, held)
    assert len(bank.modify_list(1)) == 2
    # index targets: the arg-max of the one-hot where the byte is in the palette, ignore_index elsewhere
    bank.bank[0, 1, :2] = 17
    bank.bank[0, 2, 3, 3] = 255
    idx = [0, 1, 2, st[-1] - 1, 1]
    for ignore in (255, -100):
        t = bank.targets(idx, 1, index=True, ignore_index=ignore)
        oh = bank.targets(idx, 1).numpy()
        assert t.dtype == torch.int64 and tuple(t.shape) == (5,) + init.shape[1:]
        known = oh.sum(1) == 1
        assert np.array_equal(t.numpy()[known], oh.argmax(1)[known]) and (t.numpy()[~known] == ignore).all()
        assert (~known).sum() == 4 * init.shape[2] + 1
    out = bank.targets([-1, st[-1], 0], 2, index=True, ignore_index=9).numpy()
    assert (out[:2] == 9).all() and (out[2] != 9).all()
    assert torch.equal(bank.targets(idx, 1), PseudoLabelBank(bank.bank[0], st, []).targets(idx, 1))    # the default is unchanged


def test_arguments():
    from aide_amd.labelbank import PseudoLabelBank
    from aide_amd.inference import evaluate_label_maps
    z = np.zeros((2, 4, 4), np.uint8)
    for kw in (dict(num_classes=3), dict(num_classes=5, palette=(0, 63, 63, 126, 189)), dict(num_classes=1, palette=(0,)),
               dict(num_classes=2, palette=(0, 63, 126))):
        with pytest.raises(ValueError):
            PseudoLabelBank(z, [0, 2], [], **kw)
    for kw in (dict(num_classes=3), dict(num_classes=3, palette=(0, 63)), dict(num_classes=3, palette=(0, 63, 63)),
               dict(palette=(0, 63))):
        with pytest.raises(ValueError):
            evaluate_label_maps(z, [0, 2], z, **kw)
    with pytest.raises(ValueError):
        evaluate_label_maps(z, [0, 2], z, num_classes=9, palette=tuple(range(9)))
    with pytest.raises(RuntimeError):
        PseudoLabelBank(z, [0, 2], []).class_dice()
