"""Host side of the per-class largest-component filter (aide_amd.inference.keep_largest_per_class, include/aide_hip.h
aide_keep_largest_cc3d_classes): the numpy path is the definition the device is held to, so it is checked here against an
independent flood fill (lcc_cases.flood_fill) on every case of lcc_cases; the C ABI rejects bad arguments before any launch."""
import subprocess

import numpy as np
import pytest
import torch

import lcc_cases

NEW = ('aide_lcc3d_classes_ws_bytes', 'aide_keep_largest_cc3d_classes', 'aide_lcc3d_classes_batched_ws_bytes',
       'aide_keep_largest_cc3d_classes_batched')
CASES = lcc_cases.cases()


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


@pytest.mark.parametrize('index', range(len(CASES)), ids=[c[0] for c in CASES])
def test_numpy_path_equals_flood_fill(index):
    from aide_amd.inference import keep_largest_per_class
    name, vol, c = CASES[index]
    want, want_stats = lcc_cases.flood_fill(vol, c)
    got, stats = keep_largest_per_class(vol, c, stats=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == vol.shape
    assert stats.dtype == np.int64 and stats.shape == (c, 3)
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert np.array_equal(stats, want_stats), (name, stats, want_stats)
    assert np.array_equal(keep_largest_per_class(vol, c), got)                          # without stats: the volume alone
    assert np.array_equal(keep_largest_per_class(torch.from_numpy(vol.copy()), c), got)  # a CPU tensor keeps the host path


def test_cases_are_what_they_claim():
    """the properties the case list is built for, stated on the flood fill's result"""
    by = {name: (vol, c) for name, vol, c in CASES}
    vol, c = by['serpentine']
    out, st = lcc_cases.flood_fill(vol, c)
    assert st[2].tolist() == [1, int((vol == 2).sum()), int((vol == 2).sum())]           # one component through all tiles
    assert st[1, 0] == 2 and st[3, 0] == 2 and st[1, 2] < st[2, 2] and st[3, 2] < st[2, 2]
    assert {(z // 4, y // 16, x // 16) for z, y, x in zip(*np.nonzero(vol == 2))} == \
        {(a, b, e) for a in range(3) for b in range(3) for e in range(3)}
    vol, c = by['ties']
    out, st = lcc_cases.flood_fill(vol, c)
    assert out[0, 0, 20] == 1 and out[5, 17, 0] == 0                                      # A: first in (i0, i1, i2) order
    assert out[0, 4, 17] == 3 and out[2, 8, 20] == 0
    assert st[1].tolist() == [2, 24, 12] and st[2].tolist() == [1, 12, 12] and st[3].tolist() == [2, 6, 3]
    assert out[3, 5, 30] == 2 and int((out == 2).sum()) == 12                             # classes do not compete
    assert st[4].tolist() == [3, 3, 1] and out[0, 19, 39] == 4
    vol, c = by['ties permuted']
    assert not vol.flags['C_CONTIGUOUS'] and vol.shape == (40, 9, 20)
    out, st = lcc_cases.flood_fill(vol, c)
    assert out[0, 5, 17] == 1 and out[20, 0, 0] == 0                                      # B: first in (i2, i0, i1) order
    vol, c = by['class absent']
    assert lcc_cases.flood_fill(vol, c)[1][2].tolist() == [0, 0, 0] and not (vol == 2).any()
    vol, c = by['all zero']
    out, st = lcc_cases.flood_fill(vol, c)
    assert not out.any() and not st.any()
    vol, c = by['out of range']
    out, st = lcc_cases.flood_fill(vol, c)
    assert {-3, 5, 7} <= set(np.unique(vol).tolist()) and set(np.unique(out).tolist()) == {0, 1, 2, 3, 4}
    vol, c = by['adjacent']
    out, st = lcc_cases.flood_fill(vol, c)
    assert st[:, 0].tolist() == [0, 1, 2, 1, 0] and out[4, 19, 10] == 0 and out[0, 0, 15] == 1 and out[0, 0, 16] == 2
    vol, c = by['eight classes']
    assert c == 8 and (lcc_cases.flood_fill(vol, c)[1][1:, 2] > 0).all()


def test_two_classes_is_the_binary_filter():
    from aide_amd.inference import keep_largest_per_class, keep_largest_connected_components
    binary = [(name, vol) for name, vol, c in CASES if c == 2]
    assert len(binary) >= 3
    for name, vol in binary + [('zeros', np.zeros((3, 4, 5), np.int64)), ('ones', np.ones((2, 3, 4), np.int64))]:
        got = keep_largest_per_class(vol, 2)
        assert got.tobytes() == keep_largest_connected_components(vol).tobytes(), name


def test_batched_numpy_equals_per_case():
    from aide_amd.inference import keep_largest_batched, keep_largest_per_class
    rng = np.random.RandomState(3)
    start = [0, 1, 6, 6, 15]                                                            # S_k = 1, 5, 0, 9
    lab = rng.randint(0, 5, (15, 17, 33)).astype(np.int64)
    out, stats = keep_largest_batched(lab, start, num_classes=5, stats=True)
    assert out.dtype == np.uint8 and out.shape == lab.shape and stats.shape == (4, 5, 3) and stats.dtype == np.int64
    for k, (a, b) in enumerate(zip(start, start[1:])):
        if b == a:
            assert not stats[k].any()
            continue
        want, st = keep_largest_per_class(lab[a:b].transpose(1, 2, 0), 5, stats=True)
        assert np.array_equal(out[a:b].transpose(1, 2, 0), want) and np.array_equal(stats[k], st), k
    assert np.array_equal(keep_largest_batched(lab, start, num_classes=5), out)
    # the default is still the one-blob filter
    from aide_amd.inference import keep_largest_connected_components
    one = keep_largest_batched(lab, start)
    assert set(np.unique(one).tolist()) <= {0, 1}
    assert np.array_equal(one[1:6].transpose(1, 2, 0), keep_largest_connected_components(lab[1:6].transpose(1, 2, 0)))


def test_entry_points_declared_and_exported(built):
    from aide_amd._lib import lib, parse_header
    protos = parse_header()
    header = open(__import__('aide_amd._lib', fromlist=['HEADER']).HEADER).read()
    out = subprocess.run(['nm', '-D', '--defined-only', built], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW:
        assert name in header and name in protos and name in lib.protos and name in exported, name
    assert len(protos['aide_lcc3d_classes_ws_bytes'][1]) == 2 and len(protos['aide_keep_largest_cc3d_classes'][1]) == 12
    assert len(protos['aide_lcc3d_classes_batched_ws_bytes'][1]) == 3
    assert len(protos['aide_keep_largest_cc3d_classes_batched'][1]) == 11


def test_entry_points_reject_without_launch(built):
    """answered on the host before any HIP call: every pointer is null here"""
    from aide_amd._lib import lib
    assert lib.aide_lcc3d_classes_ws_bytes(2 ** 31, 5) == 0
    assert lib.aide_lcc3d_classes_ws_bytes(-1, 5) == 0
    for c in (-1, 0, 1, 9, 256):
        assert lib.aide_lcc3d_classes_ws_bytes(1000, c) == 0
        assert lib.aide_lcc3d_classes_batched_ws_bytes(1000, 3, c) == 0
    for c in range(2, 9):
        assert lib.aide_lcc3d_classes_ws_bytes(1000, c) >= 8 * 1000 + 16 + 8 * c
        assert lib.aide_lcc3d_classes_batched_ws_bytes(1000, 3, c) >= 8 * 1000 + 16 + 8 * 3 * c
    assert lib.aide_lcc3d_classes_batched_ws_bytes(2 ** 31, 3, 5) == 0
    assert lib.aide_lcc3d_classes_batched_ws_bytes(1000, 65536, 5) == 0
    keep = lib.aide_keep_largest_cc3d_classes
    assert keep(None, 4, 4, 4, 16, 4, 1, 5, None, None, None, None) < 0                   # null pointers
    assert keep(None, 4, 4, 4, 16, 4, 1, 1, None, None, None, None) < 0                   # num_classes
    assert keep(None, 4, 4, 4, 16, 4, 1, 9, None, None, None, None) < 0
    assert keep(None, 0, 4, 4, 16, 4, 1, 9, None, None, None, None) < 0                   # ... also for an empty volume
    assert keep(None, 2 ** 16, 2 ** 15, 1, 2 ** 15, 1, 1, 5, None, None, None, None) < 0  # 2^31 voxels
    assert keep(None, -1, 4, 4, 16, 4, 1, 5, None, None, None, None) < 0
    assert keep(None, 0, 4, 4, 16, 4, 1, 5, None, None, None, None) == 0                  # empty: nothing to do
    batched = lib.aide_keep_largest_cc3d_classes_batched
    assert batched(None, None, 3, 15, 17, 33, 5, None, None, None, None) < 0
    assert batched(None, None, 3, 15, 17, 33, 1, None, None, None, None) < 0
    assert batched(None, None, 65536, 15, 17, 33, 5, None, None, None, None) < 0
    assert batched(None, None, 3, 2 ** 16, 2 ** 15, 1, 5, None, None, None, None) < 0
    assert batched(None, None, 0, 15, 17, 33, 5, None, None, None, None) == 0


def test_python_argument_errors():
    from aide_amd.inference import keep_largest_per_class, keep_largest_batched, predict_case
    vol = np.zeros((2, 3, 4), np.int64)
    for c in (1, 9):
        with pytest.raises(RuntimeError):
            keep_largest_per_class(vol, c)
        with pytest.raises(RuntimeError):
            keep_largest_batched(vol, [0, 2], num_classes=c)
    with pytest.raises(TypeError):
        predict_case(None, None, keep_largest='per_class')
    with pytest.raises(RuntimeError):
        predict_case(None, None, keep_largest='per_class', num_classes=9)
