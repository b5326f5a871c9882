"""The numpy path of aide_amd.labelbank.ImageLabelBank against fixture g24 (tools/gen_golden_image_refresh.py: the reference's
own `if (epoch + 1) <= args.warmup_epoch or ...` statements and `Dice2d` of trainbreast_dataset3_proposed_272cases25labeled.py
and trainkidney_proposed_mask1.py, and the loaders' decoding of what they write).  Everything here is integer or a single
fp64 division: comparisons are exact."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g24_image_refresh.npz')
KEYS = ['breast12', 'kidney12', 'breast3', 'kidney3']


@pytest.fixture(scope='module')
def g24():
    return np.load(GOLD)


def make_image_bank(g, key, device=None):
    from aide_amd.labelbank import ImageLabelBank
    orig = g[key + '/orig']
    if device is not None:
        orig = torch.from_numpy(orig).to(device)
    ids = list(zip(g[key + '/ids_a'].tolist(), g[key + '/ids_b'].tolist()))
    return ImageLabelBank(orig, labelled=g[key + '/labelled'].tolist(), form=str(g[key + '/form']),
                          update_percent=float(g[key + '/update_percent']), device=device, image_ids=ids)


def follow_fixture(g, key, device=None):
    """runs a bank through the recorded epochs of a scenario and compares everything the fixture holds -> the bank"""
    from aide_amd.labelbank import refresh_gate
    bank = make_image_bank(g, key, device)
    K = bank.K
    warm = int(g[key + '/warmup'])
    assert bank.n_select == int(float(g[key + '/update_percent']) * K)
    for j in range(int(g[key + '/n_epochs'])):
        pre = '%s/e%d' % (key, j)
        epoch = int(g[pre + '/epoch'])
        labels = [g['%s/gen%d' % (pre, n)] for n in (1, 2)]
        if device is not None:
            labels = [torch.from_numpy(a).to(device) for a in labels]
        wrote = bank.refresh_from_labels(labels[0], labels[1], epoch, warm)
        assert wrote == refresh_gate(epoch, warm) == bool(g[pre + '/logged'])
        dice = bank.image_dice()
        assert dice.dtype == torch.float32 and tuple(dice.shape) == (2, K) and not dice.isnan().any()
        for n in (1, 2):
            ref = g['%s/dice%d' % (pre, n)]
            assert np.array_equal(dice[n - 1].numpy().view(np.uint32), ref.view(np.uint32))
            if wrote:       # the reference's sort is not stable: the SET is the fact (the generator asserts a clean boundary)
                assert bank.written_images(n) == g['%s/written%d' % (pre, n)].tolist()
            plane = bank.bank[n - 1]
            assert np.array_equal(plane.cpu().numpy() if device is not None else plane, g['%s/plane%d' % (pre, n)])
            t = bank.targets(np.arange(K), n)
            assert t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), g['%s/target%d' % (pre, n)].astype(np.int64))
            idx = [K - 1, 0, 0, K // 2, K, -1]
            sub = bank.targets(idx, n).cpu()
            assert torch.equal(sub[:4], t.cpu()[idx[:4]]) and not sub[4:].any()
            assert bank.modify_count(n) == int(float(g[key + '/update_percent']) * K)
    return bank


def test_fixture_covers_the_cases(g24):
    g = g24
    assert g['scenarios'].tolist() == KEYS
    for key, n_sel in (('breast12', 3), ('kidney12', 4)):
        assert [int(g['%s/e%d/epoch' % (key, j)]) + 1 for j in range(3)] == [3, 25, 30] and int(g[key + '/warmup']) == 20
        assert int(float(g[key + '/update_percent']) * 12) == n_sel
        d = g[key + '/e0/dice1']
        assert np.count_nonzero(d == 0.0) >= 2 and d[4] == d[5]                      # ties, at 0.0 and elsewhere
        assert int(g[key + '/e1/logged']) == 0 and len(g[key + '/e1/written1']) == 0
        assert len(g[key + '/e0/written1']) < n_sel                                  # an empty prediction (or a label) was skipped
    assert 0 in g['breast12/labelled'] and g['breast12/e0/dice1'][0] == 0.0 and 0 not in g['breast12/e0/written1']
    assert g['kidney12/orig'][6].min() == 255 and g['kidney12/e2/plane1'][6].min() == 0 and not g['kidney12/e2/target1'][6].any()
    assert len(g['breast3/e0/files']) == 0 and len(g['kidney3/e0/files']) == 0


@pytest.mark.parametrize('key', KEYS)
def test_numpy_bank_follows_the_reference(g24, key, tmp_path):
    g = g24
    bank = follow_fixture(g, key)
    last = '%s/e%d' % (key, int(g[key + '/n_epochs']) - 1)
    root = str(tmp_path)
    got = {}
    paths = bank.export(root, writer=(lambda p, a: got.__setitem__(p, a)) if bank.form == 'kidney' else None)
    assert sorted(os.path.relpath(p, root) for p in paths) == sorted(g[last + '/files'].tolist())
    for p in paths:
        n = int(p.split('_net')[1][0])
        rel = os.path.relpath(p, root).split(os.sep)
        k = [i for i in range(bank.K) if g[key + '/ids_a'][i] == rel[0] and rel[1].startswith(
            ('%s_depth%s_net' % (rel[0], g[key + '/ids_b'][i])) if bank.form == 'breast' else g[key + '/ids_b'][i] + '_net')]
        assert len(k) == 1
        if bank.form == 'breast':
            from PIL import Image
            img = Image.open(p)
            assert img.mode == 'L' and np.array_equal(np.array(img), g['%s/plane%d' % (last, n)][k[0]])
        else:
            assert got[p].dtype == np.int64 and got[p].shape == (1, bank.H, bank.W)
            assert np.array_equal(got[p][0], g['%s/plane%d' % (last, n)][k[0]])


def _square(K, h, rows):
    m = np.zeros((K, h, h), np.uint8)
    for k, r in enumerate(rows):
        m[k, :r] = 1
    return m


def test_network_2_is_scored_before_network_1_is_rewritten():
    """breast: network 2's target is network 1's plane as it was BEFORE this refresh.  Scoring network 2 after network 1's
    update (the order of PseudoLabelBank.refresh_from_labels) would write a different set."""
    from aide_amd.labelbank import ImageLabelBank
    K, h = 4, 8
    orig = _square(K, h, [4, 4, 4, 4]) * 255
    l1 = _square(K, h, [1, 4, 4, 4])                # network 1: image 0 is its worst -> rewritten with one row
    l2 = _square(K, h, [1, 2, 3, 4])                # network 2: against the OLD plane image 0 is its worst (2*8/40) ...
    bank = ImageLabelBank(orig, form='breast', update_percent=0.25)
    assert bank.n_select == 1 and bank.refresh_from_labels(l1, l2, 0, 5)
    d = bank.image_dice().numpy()
    assert d[1, 0] == np.float32(2 * 8 / 40.0) and bank.written_images(1) == [0] and bank.written_images(2) == [0]
    # ... while against the NEW plane (one row) image 0 would score 1.0 and image 1 would be the one written
    wrong = ImageLabelBank(bank.bank[0].copy(), form='breast', update_percent=0.25)
    wrong.refresh_from_labels(l1, l2, 0, 5)
    assert wrong.image_dice().numpy()[1, 0] == 1.0 and wrong.written_images(2) == [1]
    assert np.array_equal(bank.bank[1, 0], l2[0] * 255) and np.array_equal(bank.bank[1, 1:], orig[1:])
    # kidney: each network against the OTHER's plane, both from before the refresh
    kid = ImageLabelBank(orig, form='kidney', update_percent=0.25)
    kid.bank[0][:] = _square(K, h, [4, 4, 4, 1])    # network 1's plane: network 2's target
    kid.bank[1][:] = _square(K, h, [4, 1, 4, 4])    # network 2's plane: network 1's target
    full = _square(K, h, [4, 4, 4, 4])
    kid.refresh_from_labels(full, full, 0, 5)
    assert kid.written_images(1) == [1] and kid.written_images(2) == [3]
    assert np.array_equal(kid.bank[0][1], full[1]) and np.array_equal(kid.bank[1][3], full[3])      # scale 1


def test_union_zero_is_zero_and_empty_predictions_are_not_written():
    from aide_amd.inference import image_dice_rule
    from aide_amd.labelbank import ImageLabelBank
    #              N  p*t  p  t
    sums = np.array([[16, 0, 0, 0], [16, 0, 0, 5], [16, 0, 3, 0], [16, 2, 4, 4], [16, 4, 4, 4], [16, 1, 4, 4]])
    dice, rank, written = image_dice_rule(sums, n_select=4)
    assert dice.dtype == np.float32 and not np.isnan(dice).any() and dice[:3].tolist() == [0.0, 0.0, 0.0]
    assert rank.tolist() == [0, 1, 2, 4, 5, 3]              # the ties at 0.0 by the lower index (this project's rule)
    assert written.tolist() == [0, 0, 1, 0, 0, 1]           # 0 and 1 are selected and skipped: their predictions are empty
    _, _, w = image_dice_rule(sums, labelled=[0, 0, 1, 0, 0, 0], n_select=4)
    assert w.tolist() == [0, 0, 0, 0, 0, 1]
    # the fp64 division, rounded once
    big = np.array([[0, 16777217, 16777217, 50331653]])
    assert image_dice_rule(big)[0][0] == np.float32(np.float64(2 * 16777217) / np.float64(16777217 + 50331653))
    # through the bank: the selected empty prediction leaves the plane alone, and its slot is not handed on
    orig = _square(4, 4, [2, 2, 2, 2]) * 255
    lab = _square(4, 4, [0, 1, 2, 2])
    bank = ImageLabelBank(orig, form='breast', update_percent=0.25)
    bank.refresh_from_labels(lab, lab, 0, 5)
    assert bank.rank[0].tolist() == [0, 1, 2, 3] and bank.written.tolist() == [[0, 0, 0, 0]] * 2
    assert np.array_equal(bank.bank[0], orig) and bank.modify_count(1) == 1
    # kidney ignores `labelled`; breast honours it
    for form, want in (('breast', []), ('kidney', [1])):
        b = ImageLabelBank(orig, labelled=[1], form=form, update_percent=0.5)
        b.refresh_from_labels(lab, lab, 0, 5)
        assert b.written_images(1) == want


@pytest.mark.parametrize('K,up,want', [(12, 0.25, 3), (12, 0.4, 4), (3, 0.25, 0), (10, 0.7, 7), (100, 0.29, 28), (7, 1.0, 7)])
def test_n_select_truncates_the_float_product(K, up, want):
    """int(update_percent * K) as Python computes it: 0.29 * 100 = 28.999999999999996 -> 28, not round(29)"""
    from aide_amd.labelbank import ImageLabelBank
    bank = ImageLabelBank(np.zeros((K, 2, 2), np.uint8), form='kidney', update_percent=up)
    assert bank.n_select == want == int(up * K)


def test_kidney_gate_comes_from_the_original_masks():
    from aide_amd.labelbank import ImageLabelBank
    orig = np.zeros((3, 4, 4), np.uint8)
    orig[0, :2] = 255                                        # two values: gate open
    orig[1] = 255                                            # constant: every target of image 1 is zero
    bank = ImageLabelBank(orig, form='kidney')
    assert bank.gate_host.tolist() == [1, 0, 0]
    bank.bank[0][:] = 1
    assert bank.targets([0, 1, 2], 1).sum((1, 2)).tolist() == [16, 0, 0]
    assert ImageLabelBank(orig, form='breast').gate_host is None
