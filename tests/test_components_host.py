"""Host side of the labelled components and the lesion-wise scores (aide_amd.inference.label_components, region_table,
lesion_counts, lesion_scores, case_scores(lesions=...); include/aide_hip.h aide_label_components3d and aide_lesion_counts3d): the
numpy paths are held to the independent flood fill of components_cases on every case, and the C ABI rejects bad arguments
before any launch.  Everything is integer, so every comparison is exact."""
import subprocess

import numpy as np
import pytest
import torch

import components_cases as cc

NEW = ('aide_label_components3d_ws_bytes', 'aide_label_components3d', 'aide_lesion_counts3d_ws_bytes', 'aide_lesion_counts3d')
LABELS = cc.label_cases()
PAIRS = cc.pair_cases()
OLD_KEYS = ('Dice', 'IoU', 'TP', 'TN', 'FP', 'FN')
LESION_KEYS = ('target_blobs', 'detected', 'pred_blobs', 'matched', 'covered_voxels', 'spurious_voxels', 'sensitivity',
               'precision', 'F1')


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_cases_are_what_they_claim():
    names = [case.name for case in LABELS]
    assert len(set(names)) == len(names) and len(LABELS) >= 60
    for word in ('permuted', 'out of range', 'negative only', 'all zero', 'eight classes', 'tiny 1x1x1', 'tiny 3x3x3', 'uint8',
                 'int32'):
        assert any(word in name for name in names), word
    assert any(not case.volume.flags['C_CONTIGUOUS'] for case in LABELS)
    assert {case.volume.dtype for case in LABELS} == {np.dtype(np.int64), np.dtype(np.int32), np.dtype(np.uint8)}
    index = names.index('negative only 3x5x7 binary')          # members in the binary form, none with classes
    assert cc.label_reference(index)[1] == 1 and cc.label_reference(index + 1)[1] == 0
    index = [i for i, case in enumerate(LABELS) if case.name.startswith('out of range') and case.classes == 5][0]
    labels = cc.label_reference(index)[0]
    vol = LABELS[index].volume
    assert (labels[(vol < 1) | (vol > 4)] == 0).all() and (labels[(vol >= 1) & (vol <= 4)] > 0).all()
    names = [case.name for case in PAIRS]
    assert len(set(names)) == len(names)
    assert sum(name.startswith('random') for name in names) >= 20
    for word in ('swapped', 'permuted pred', 'all-zero pred', 'all-zero target', 'both all-zero', 'uint8 pred int32 target'):
        assert any(word in name for name in names), word
    p, t = cc.hand_pair()
    sides = cc.flood_pair(p, t, 5)
    assert sorted((area, cover) for _, area, cover in sides[0]) == sorted(
        [(12, 12), (12, 6), (12, 1), (12, 0), (4, 4), (4, 4), (80, 64), (12, 0)])
    assert sorted((area, cover) for _, area, cover in sides[1]) == sorted(
        [(12, 12), (6, 6), (2, 1), (12, 0), (12, 8), (32, 32), (32, 32), (12, 0)])
    assert cc.counts(12, 6, 0.5) and not cc.counts(12, 6, 0.5 + 2.0 ** -50) and not cc.counts(12, 0, 0.0)


@pytest.mark.parametrize('index', range(len(LABELS)), ids=[c.name for c in LABELS])
def test_label_components_host_equals_flood_fill(index):
    from aide_amd.inference import label_components, region_table
    case = LABELS[index]
    want, want_count, want_props = cc.label_reference(index)
    before = case.volume.copy()
    labels, count, props = label_components(case.volume, case.classes, props=True)
    assert labels.dtype == np.int32 and labels.shape == case.volume.shape and labels.flags['C_CONTIGUOUS']
    assert count.dtype == np.int64 and count.shape == (1,) and int(count[0]) == want_count
    assert props.dtype == np.int64 and props.shape == (65536, 12)
    assert np.array_equal(labels, want), (case.name, int((labels != want).sum()))
    assert np.array_equal(props, want_props), case.name
    assert np.array_equal(case.volume, before)
    alone = label_components(torch.from_numpy(np.array(case.volume)), case.classes)      # a CPU tensor, no props
    assert len(alone) == 2 and np.array_equal(alone[0], want) and int(alone[1][0]) == want_count
    table = region_table(props, count)
    assert table['count'] == want_count and len(table['area']) == want_count
    assert table['centroid'].dtype == np.float64 and table['centroid'].shape == (want_count, 3)
    for j in range(min(want_count, 40)):          # the centroid is the mean of the blob's voxel coordinates
        where = np.argwhere(want == j + 1)
        assert len(where) == table['area'][j] and np.array_equal(table['centroid'][j], where.sum(axis=0) / np.float64(len(where)))
        assert np.array_equal(table['bbox'][j], np.concatenate([where.min(axis=0), where.max(axis=0) + 1]))
        first = np.unravel_index(table['first'][j], want.shape)
        assert tuple(first) == tuple(where[0]) and case.volume[first] == table['value'][j]


def test_cap_below_the_count_host():
    from aide_amd.inference import label_components, region_table
    vol = cc.three_blobs()
    want, want_count, want_props = cc.flood_labels(vol, None, 2)
    assert want_count == 4
    labels, count, props = label_components(vol, None, props=True, max_blobs=2)
    assert np.array_equal(labels, want) and int(count[0]) == 4 and props.shape == (2, 12) and np.array_equal(props, want_props)
    assert (props[:, 1] > 0).all() and region_table(props, count)['count'] == 4 and len(region_table(props, count)['area']) == 2
    labels, count, props = label_components(vol, None, props=True, max_blobs=7)
    assert np.array_equal(props, cc.flood_labels(vol, None, 7)[2]) and not props[4:].any() and props[:4, 1].tolist() == [30, 18, 18, 7]


def test_empty_volume_host():
    from aide_amd.inference import label_components, lesion_counts
    empty = np.zeros((0, 4, 4), np.int64)
    labels, count, props = label_components(empty, 5, props=True, max_blobs=3)
    assert labels.shape == (0, 4, 4) and labels.dtype == np.int32 and count.tolist() == [0] and not props.any()
    assert not lesion_counts(empty, empty, 5, 0.5).any()


@pytest.mark.parametrize('index', range(len(PAIRS)), ids=[c.name for c in PAIRS])
def test_lesion_counts_host_equal_flood_fill(index):
    from aide_amd.inference import lesion_counts, lesion_scores, case_scores
    case = PAIRS[index]
    sides = cc.pair_reference(index)
    for overlap in cc.OVERLAPS:
        want = cc.flood_lesions(sides, case.classes, overlap)
        got = lesion_counts(case.pred, case.target, case.classes, overlap)
        assert got.dtype == np.int64 and got.shape == (case.classes or 2, 6) and np.array_equal(got, want), (case.name, overlap, got, want)
        swapped = lesion_counts(case.target, case.pred, case.classes, overlap)
        assert np.array_equal(swapped[:, :4], want[:, [2, 3, 0, 1]]), (case.name, overlap)          # the columns swap
        scores, want_scores = lesion_scores(case.pred, case.target, case.classes, overlap), cc.scores_of(want, case.classes)
        assert tuple(scores) == LESION_KEYS
        for key in LESION_KEYS:
            assert same(scores[key], want_scores[key]), (case.name, overlap, key)
            if case.classes is None:
                assert np.ndim(scores[key]) == 0
            else:
                assert scores[key].shape == (case.classes,) and scores[key].dtype == (np.int64 if key in LESION_KEYS[:6] else np.float64)
    if case.classes is None:                      # column 5 is the voxel-wise TP of the binarised volumes
        tp = case_scores((np.asarray(case.pred) != 0).astype(np.int64), (np.asarray(case.target) != 0).astype(np.int64))['TP']
        assert want[1, 4] == tp
    else:
        tp = case_scores(np.asarray(case.pred), np.asarray(case.target), case.classes)['TP']
        assert np.array_equal(want[1:, 4], tp[1:]) and want[0].tolist() == [0] * 6


def test_case_scores_with_and_without_lesions():
    from aide_amd.inference import case_scores, lesion_scores
    names = {case.name: case for case in PAIRS}
    for name in ('hand C=5', 'hand binary', 'random classes 9x40x21 0.6', 'random binary 6x33x18 0.8'):
        case = names[name]
        pred = np.asarray(case.pred) if case.classes else (np.asarray(case.pred) != 0).astype(np.int64)
        target = np.asarray(case.target) if case.classes else (np.asarray(case.target) != 0).astype(np.int64)
        old = case_scores(pred, target, case.classes)
        assert tuple(old) == OLD_KEYS             # exactly the old keys
        new = case_scores(pred, target, case.classes, lesions=0.5)
        assert tuple(new) == OLD_KEYS + tuple('lesion_' + k for k in LESION_KEYS)
        alone = lesion_scores(pred, target, case.classes, 0.5)
        for key in OLD_KEYS:
            assert same(new[key], old[key]), (name, key)
        for key in LESION_KEYS:
            assert same(new['lesion_' + key], alone[key]), (name, key)
        spaced = case_scores(pred, target, case.classes, spacing=(2.0, 1.0, 1.0), lesions=0.1)
        assert 'ASSD' in spaced and same(spaced['lesion_detected'], lesion_scores(pred, target, case.classes, 0.1)['detected'])
        assert tuple(case_scores(pred, target, case.classes, spacing=(2.0, 1.0, 1.0))) == OLD_KEYS + ('RAVD', 'ASSD', 'MSSD')
    hand = names['hand C=5']
    got = lesion_scores(hand.pred, hand.target, 5, 0.5)
    assert got['target_blobs'].tolist() == [0, 4, 2, 1, 1] and got['detected'].tolist() == [0, 4, 1, 0, 0]
    assert got['pred_blobs'].tolist() == [0, 3, 3, 2, 0] and got['matched'].tolist() == [0, 3, 3, 0, 0]
    assert np.isnan(got['sensitivity'][0]) and got['sensitivity'][1:].tolist() == [1.0, 0.5, 0.0, 0.0]
    assert np.isnan(got['precision'][4]) and np.isnan(got['F1'][3]) and got['F1'][1] == 1.0
    assert got['spurious_voxels'].tolist() == [0, 0, 0, 24, 0] and got['covered_voxels'].tolist() == [0, 26, 65, 0, 0]


def test_bad_arguments_raise():
    from aide_amd.inference import label_components, lesion_counts, lesion_scores, case_scores, region_table
    vol = cc.three_blobs()
    for bad in (0, -1, 2 ** 20 + 1, 2.0, '4', None, True):
        with pytest.raises(ValueError):
            label_components(vol, None, True, bad)
    label_components(vol, None, True, 1)
    for bad in (1, 9, 0, -2, 2.0, True, '5'):
        with pytest.raises(ValueError):
            label_components(vol, bad)
        with pytest.raises(ValueError):
            lesion_scores(vol, vol, bad)
    for bad in (-0.1, 1.5, float('nan'), float('inf'), '0.5', True, (0.5,)):
        with pytest.raises(ValueError):
            lesion_scores(vol, vol, None, bad)
        with pytest.raises(ValueError):
            lesion_counts(vol, vol, 5, bad)
        with pytest.raises(ValueError):
            case_scores(vol, vol, lesions=bad)
    assert lesion_scores(vol, vol, None, 1)['detected'] == 4 and lesion_scores(vol, vol, None, 0)['matched'] == 4
    with pytest.raises(RuntimeError):
        lesion_scores(vol, vol[:, :, :-1])
    with pytest.raises(RuntimeError):
        label_components(vol[0])
    with pytest.raises(RuntimeError):
        label_components(vol.astype(np.float32))
    with pytest.raises(TypeError):
        region_table(np.zeros((4, 11), np.int64), np.zeros(1, np.int64))
    with pytest.raises(TypeError):
        region_table(np.zeros((4, 12), np.int64), np.zeros(2, np.int64))
    with pytest.raises(TypeError):
        case_scores(vol, vol, percentiles=(95,), lesions=0.5)


def test_entry_points_declared_and_exported(built):
    from aide_amd._lib import lib, parse_header
    protos = parse_header()
    out = subprocess.run(['nm', '-D', '--defined-only', built], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW:
        assert name in protos and name in lib.protos and name in exported, name
    assert len(protos['aide_label_components3d_ws_bytes'][1]) == 1 and len(protos['aide_label_components3d'][1]) == 14
    assert len(protos['aide_lesion_counts3d_ws_bytes'][1]) == 1 and len(protos['aide_lesion_counts3d'][1]) == 16


def test_workspace_queries(built):
    from aide_amd._lib import lib
    for query in (lib.aide_label_components3d_ws_bytes, lib.aide_lesion_counts3d_ws_bytes):
        assert query(2 ** 31) == 0 and query(-1) == 0 and query(2 ** 40) == 0
        sizes = [query(n) for n in (0, 1, 2, 255, 256, 257, 1000, 4096, 10 ** 6, 2 ** 31 - 1)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
        assert query(1000) >= 12 * 1000 + 32 and query(1000) % 4 == 0 and query(2 ** 31 - 1) >= 12 * (2 ** 31 - 1)
    assert lib.aide_label_components3d_ws_bytes(10 ** 6) >= lib.aide_lesion_counts3d_ws_bytes(10 ** 6) + 4 * 977


def test_entry_points_reject_without_launch(built):
    """answered on the host before any HIP call: every device pointer is null here"""
    from aide_amd._lib import lib
    label, lesion = lib.aide_label_components3d, lib.aide_lesion_counts3d
    count = 8                                     # stands for a non-null count / out pointer: never dereferenced on these paths
    assert label(None, 4, 4, 4, 16, 4, 1, 5, None, count, None, 0, None, None) < 0               # null v / labels / ws
    assert label(None, 4, 4, 4, 16, 4, 1, 0, None, None, None, 0, None, None) < 0                # null count
    for c in (-1, 1, 9, 256):
        assert label(None, 0, 4, 4, 16, 4, 1, c, None, count, None, 0, None, None) < 0           # num_classes, also when empty
    for cap in (0, -1, 2 ** 20 + 1):
        assert label(None, 0, 4, 4, 16, 4, 1, 5, None, count, count, cap, None, None) < 0        # props with a bad cap
    assert label(None, 2 ** 16, 2 ** 15, 1, 2 ** 15, 1, 1, 5, None, count, None, 0, None, None) < 0   # 2^31 voxels
    assert label(None, -1, 4, 4, 16, 4, 1, 5, None, count, None, 0, None, None) < 0
    assert lesion(None, 16, 4, 1, None, 16, 4, 1, 4, 4, 4, 5, 0.5, count, None, None) < 0        # null volumes / ws
    assert lesion(None, 16, 4, 1, None, 16, 4, 1, 0, 4, 4, 5, 0.5, None, None, None) < 0         # null out
    for c in (-1, 1, 9, 256):
        assert lesion(None, 16, 4, 1, None, 16, 4, 1, 0, 4, 4, c, 0.5, count, None, None) < 0
    for overlap in (-0.5, 1.0 + 2.0 ** -40, float('nan'), float('inf')):
        assert lesion(None, 16, 4, 1, None, 16, 4, 1, 0, 4, 4, 5, overlap, count, None, None) < 0
    assert lesion(None, 16, 4, 1, None, 16, 4, 1, 2 ** 16, 2 ** 15, 1, 5, 0.5, count, None, None) < 0
