"""The three host rules of the pseudo-label refresh -- `case_dice_rule`, `case_dice_rule_classes`, `image_dice_rule` of
aide_amd/inference.py -- share one ranking (`_rank_select`) and differ in the score and the eligibility.  Where the
definitions coincide (sum p > 0 in every row, C = 2 counts of the same maps) they give the same dice bits, ranks and flags;
where sum p + sum t = 0 the case rules give NaN, ranked last, and the image rule 0.0, ranked first.  Exact: no tolerance."""
import numpy as np
import pytest

import refresh_shared_cases as rc
from aide_amd.inference import case_dice_rule, case_dice_rule_classes, image_dice_rule


@pytest.mark.parametrize('k', [1, 2, 37, 1025])
def test_rules_agree_where_they_coincide(k):
    sums, labelled, n = rc.shared_sums(k, k)
    assert (sums[:, 2] > 0).all()
    for lab, n_select in ((labelled, n), (None, n), (labelled, 0), (labelled, k + 3)):
        binary = case_dice_rule(sums, lab, n_select)
        classes = case_dice_rule_classes(rc.counts_c2(sums), lab, n_select)[1:]
        image = image_dice_rule(sums, lab, n_select)
        for name, a, b, c in zip(('dice', 'rank', 'flag'), binary, classes, image):
            assert rc.same_bits(a, b) and rc.same_bits(a, c), (k, n_select, name)
        assert sorted(binary[1]) == list(range(k))
    if k > 1:
        dice, rank, sel = case_dice_rule(sums, labelled, n)
        assert rc.boundary_tie(dice, rank, n)                              # the generator's tie is really there
        if k > 2:
            assert len(np.unique(dice)) < k // 2 and labelled.any()        # many equal scores, some labelled rows
        order = np.argsort(rank)
        assert order[n - 1] < order[n]                                     # ... and goes to the lower index
        assert np.array_equal(sel, (rank < n) & (labelled == 0))


@pytest.mark.parametrize('k', [8, 37, 1025])
def test_empty_rows(k):
    sums, labelled, n = rc.shared_sums(k + 1, k, zero_rows=True)
    empty = sums[:, 2] + sums[:, 3] == 0
    assert 0 < empty.sum() == k // 8
    dice, rank, sel = case_dice_rule(sums, labelled, n)
    cdice, crank, csel = case_dice_rule_classes(rc.counts_c2(sums), labelled, n)[1:]
    assert rc.same_bits(dice, cdice) and rc.same_bits(rank, crank) and rc.same_bits(sel, csel)
    assert np.isnan(dice[empty]).all() and not np.isnan(dice[~empty]).any()
    # NaN is ranked last, the NaN rows among themselves by their index
    assert np.array_equal(rank[empty], k - empty.sum() + np.arange(empty.sum()))
    assert not sel[empty].any()
    assert rc.boundary_tie(dice, rank, n)
    idice, irank, iwritten = image_dice_rule(sums, labelled, n)
    assert (idice[empty] == 0.0).all() and rc.same_bits(idice[~empty], dice[~empty])
    # 0.0 with sum p + sum t = 0 is the least score there is: these rows are ranked first, by their index, and never written
    zero = idice == 0.0
    assert np.array_equal(irank[zero], np.arange(zero.sum()))
    assert not iwritten[empty].any()
    assert np.array_equal(iwritten, (irank < n) & (sums[:, 2] > 0) & (labelled == 0))
