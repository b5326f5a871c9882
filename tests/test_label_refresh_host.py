"""The numpy path of aide_amd.labelbank.PseudoLabelBank against fixture g23 (tools/gen_golden_label_refresh.py: the
reference's own `if (epoch + 1) <= args.warmup_epoch or ...` statement, trainchaos_proposed_30cases1labeled.py:528-575, and the
loader's decoding of the files it writes).  Everything here is integer or a single fp64 division: comparisons are exact."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_label_refresh.npz')


@pytest.fixture(scope='module')
def g23():
    return np.load(GOLD)


def make_bank(g, key, device=None):
    from aide_amd.labelbank import PseudoLabelBank
    init = g[key + '/init']
    if device is not None:
        init = torch.from_numpy(init).to(device)
    return PseudoLabelBank(init, g[key + '/slice_start'].tolist(), g[key + '/labelled'].tolist(),
                           case_ids=g[key + '/case_ids'].tolist(), device=device)


def expected_written(g, key, j):
    """(case id, stem, net) of the files the reference had written after recorded epoch j"""
    return sorted(str(f) for f in g['%s/e%d/files' % (key, j)].tolist())


def test_fixture_covers_the_cases(g23):
    g = g23
    assert [int(g['k9/e%d/epoch' % j]) + 1 for j in range(3)] == [3, 25, 30] and int(g['k9/warmup']) == 20
    lab_ids = set(g['k9/case_ids'][g['k9/labelled']].tolist())
    mods = [set(g['k9/e%d/modify%d' % (j, n)].tolist()) for j in (0, 2) for n in (1, 2)]
    assert all(len(m) == 2 for m in mods) and any(m & lab_ids for m in mods) and mods[0] != mods[1]
    assert np.isnan(g['k9/e0/dice1']).any()
    d = g['k9/e0/dice1']
    assert len(np.unique(d[~np.isnan(d)])) < np.count_nonzero(~np.isnan(d))        # a tie is present
    assert int(g['k9/e1/logged1']) == 0 and len(g['k3/e0/files']) == 0


@pytest.mark.parametrize('key', ['k9', 'k3'])
def test_numpy_bank_follows_the_reference(g23, key, tmp_path):
    from aide_amd.labelbank import refresh_gate
    g = g23
    bank = make_bank(g, key)
    ids = g[key + '/case_ids'].tolist()
    start = g[key + '/slice_start'].tolist()
    stems = g[key + '/stems'].tolist()
    warm = int(g[key + '/warmup'])
    assert bank.n_select == int(0.25 * len(ids))
    for j in range(int(g[key + '/n_epochs'])):
        pre = '%s/e%d' % (key, j)
        epoch = int(g[pre + '/epoch'])
        wrote = bank.refresh_from_labels(g[pre + '/gen1'], g[pre + '/gen2'], epoch, warm, keep_largest=False)
        assert wrote == refresh_gate(epoch, warm) == bool(g[pre + '/logged1'])
        dice = bank.case_dice()
        assert dice.dtype == torch.float32 and tuple(dice.shape) == (2, len(ids))
        for n in (1, 2):
            ref = g['%s/dice%d' % (pre, n)]
            got = dice[n - 1].numpy()
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            assert np.array_equal(got[~np.isnan(ref)].view(np.uint32), ref[~np.isnan(ref)].view(np.uint32))
            if wrote:       # the reference's sort is not stable: the SET is the fact (the generator asserts a clean boundary)
                assert sorted(bank.modify_list(n)) == sorted(g['%s/modify%d' % (pre, n)].tolist())
            # the bank holds the bytes of the PNGs the loader would open, the targets are its one-hot
            assert np.array_equal(bank.bank[n - 1], g['%s/plane%d' % (pre, n)])
            t = bank.targets(np.arange(start[-1]), n)
            assert t.dtype == torch.int64 and np.array_equal(t.numpy(), g['%s/onehot%d' % (pre, n)].astype(np.int64))
        # export_png: the same files, decoding to the same planes
        root = str(tmp_path / ('%s_%d' % (key, j)))
        os.makedirs(root)
        paths = bank.export_png(root, stems)
        assert sorted(os.path.relpath(p, root) for p in paths) == expected_written(g, key, j)
        from PIL import Image
        for p in paths:
            rel = os.path.relpath(p, root)
            cid, name = rel.split(os.sep)
            k, n = ids.index(int(cid)), int(name[-5])
            s = start[k] + stems[start[k]:start[k + 1]].index(name[:-len('_net1.png')])
            img = Image.open(p)
            assert img.mode == 'L' and np.array_equal(np.array(img), g['%s/plane%d' % (pre, n)][s])
    lab = g[key + '/labelled'].tolist()
    for k in lab:                                          # a labelled case's planes never change
        assert np.array_equal(bank.bank[:, start[k]:start[k + 1]], np.stack([g[key + '/init'][start[k]:start[k + 1]]] * 2))


def test_gate():
    from aide_amd.labelbank import refresh_gate
    open_ = [e for e in range(45) if refresh_gate(e, 20)]
    assert open_ == list(range(20)) + [29, 39]
    assert [e for e in range(25) if refresh_gate(e, 0)] == [9, 19]


def test_skipped_slot_is_not_handed_on():
    """a labelled case inside the worst quarter is skipped and the next case does NOT take its place (:535)"""
    from aide_amd.inference import case_dice_rule
    sums = np.array([[8, 1, 4, 4], [8, 0, 4, 4], [8, 2, 4, 4], [8, 3, 4, 4], [8, 4, 4, 4], [8, 4, 4, 4], [8, 4, 4, 4], [8, 4, 4, 4]])
    dice, rank, sel = case_dice_rule(sums, labelled=[0, 1, 0, 0, 0, 0, 0, 0], n_select=2)
    assert rank.tolist() == [1, 0, 2, 3, 4, 5, 6, 7] and sel.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_boundary_tie_rule():
    """this project's rule where the reference has none: equal Dice at the boundary -> the lower case index; NaN last"""
    from aide_amd.inference import case_dice_rule
    sums = np.array([[4, 1, 2, 2], [4, 0, 0, 0], [4, 1, 2, 2], [4, 1, 2, 2], [4, 0, 0, 0]])
    dice, rank, sel = case_dice_rule(sums, n_select=2)
    assert np.isnan(dice[[1, 4]]).all() and rank.tolist() == [0, 3, 1, 2, 4] and sel.tolist() == [1, 0, 1, 0, 0]
    assert dice.dtype == np.float32 and dice[0] == np.float32(np.float64(2) / np.float64(4))


def test_numpy_path_filters_per_case():
    """refresh_from_labels with keep_largest: a blob that touches the next case's first slice at the same (h, w) stays two
    blobs, and the smaller part of a case is dropped before it is scored and written"""
    from aide_amd.labelbank import PseudoLabelBank
    init = np.zeros((4, 8, 8), np.uint8)
    init[:, 1:4, 1:4] = 63
    lab = np.zeros((4, 8, 8), np.int64)
    lab[1, 1:4, 1:4] = 1                 # case 0: slices 0-1; 9 voxels in its last slice ...
    lab[2, 1:3, 1:3] = 1                 # ... case 1: slices 2-3; 4 voxels right behind them, and 6 apart
    lab[3, 5:7, 4:7] = 1
    bank = PseudoLabelBank(init, [0, 2, 4, 4, 4], [])
    assert bank.n_select == 1
    bank.refresh_from_labels(lab, lab, 0, 5)
    d = bank.case_dice().numpy()
    assert d[0, 0] == np.float32(2 * 9 / (9 + 18)) and d[0, 1] == np.float32(0.0) and np.isnan(d[0, 2:]).all()
    assert bank.selected[0].tolist() == [0, 1, 0, 0]
    want = init.copy()
    want[2:4] = 0
    want[3, 5:7, 4:7] = 63
    assert np.array_equal(bank.bank[0], want) and np.array_equal(bank.bank[1], want)
