"""Host side of the case post-processing (aide_amd.inference.keep_components and fill_holes, include/aide_hip.h
aide_keep_components3d and aide_fill_holes3d): the numpy paths are held to the independent flood fill of postprocess_cases on
every case, fill_holes also to scipy.ndimage.binary_fill_holes, keep_components at top_k = 1, min_voxels = 1 to the two existing
host filters; the C ABI rejects bad arguments before any launch."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import postprocess_cases as pc

NEW = ('aide_components3d_ws_bytes', 'aide_keep_components3d', 'aide_fill_holes3d_ws_bytes', 'aide_fill_holes3d')
CASES = pc.cases()
HOLES, COMPONENTS = CASES['holes'], CASES['components']


@pytest.fixture(scope='module')
def built():
    from aide_amd.build import build
    return build(verbose=False)


def test_cases_are_what_they_claim():
    """the properties the hand cases are built for, stated on the flood fill's result"""
    holes = {case.name: index for index, case in enumerate(HOLES)}

    def fate(name, axis=None):
        return pc.holes_reference(holes[name], axis)[2]

    def filled(name, axis=None):
        out, stats, _ = pc.holes_reference(holes[name], axis)
        return int(stats[:, 1].sum())

    assert fate('centre') == dict(filled=1, mixed=0, open=0) and filled('centre') == 1
    assert pc.holes_reference(holes['centre classes'], None)[0][1, 1, 1] == 3
    for name in ('cavity across tiles', 'cavity across tiles classes'):
        assert fate(name) == dict(filled=1, mixed=0, open=0) and filled(name) == 5 * 10 * 24
    assert fate('channel') == dict(filled=0, mixed=0, open=1) and filled('channel', 0) == 4 * 10 * 24
    out = pc.holes_reference(holes['diagonal'], None)[0]
    assert out[1, 1, 1] == 1 and out[3, 4, 4] == 1 and out[0, 0, 0] == 0 and out[4, 5, 4] == 0
    assert fate('island same class') == dict(filled=1, mixed=0, open=0)
    assert fate('island other class') == dict(filled=0, mixed=1, open=0)
    assert fate('island other class binary') == dict(filled=1, mixed=0, open=0)
    assert fate('two-class shell') == dict(filled=0, mixed=1, open=0)
    assert fate('out of range neighbour') == dict(filled=0, mixed=1, open=0)
    assert fate('negative neighbour') == dict(filled=0, mixed=1, open=0)
    assert fate('out of range neighbour binary') == dict(filled=1, mixed=0, open=0)
    assert fate('tube') == dict(filled=0, mixed=0, open=1)
    assert fate('tube', 2) == dict(filled=40, mixed=0, open=0) and fate('tube', 0) == dict(filled=0, mixed=0, open=2)
    assert not pc.holes_reference(holes['all zero'], None)[0].any()
    assert fate('all foreground') == dict(filled=0, mixed=0, open=0)
    for name in ('blocky 7', 'blocky 8'):                   # both kinds of hole, many of each
        assert fate(name)['filled'] > 100 and fate(name)['mixed'] > 100, fate(name)
    for name in ('blocky permuted', 'cavity permuted', 'uint8 permuted'):
        assert not HOLES[holes[name]].volume.flags['C_CONTIGUOUS']
    assert HOLES[holes['uint8 classes']].volume.dtype == np.uint8 and 253 in HOLES[holes['uint8 classes']].volume
    for index, case in enumerate(HOLES):                    # a slice rule fills at least what 3-D fills, more on the random volumes
        if case.classes is None:
            flat = [int(pc.holes_reference(index, axis)[0].sum()) for axis in pc.AXES]
            assert flat[0] <= flat[1] and flat[0] <= flat[2], case.name
            if case.name.startswith('random') and 1 not in case.volume.shape:
                assert flat[0] < flat[1] and flat[0] < flat[2], case.name
    comps = {case.name: index for index, case in enumerate(COMPONENTS)}

    def kept(name):
        return pc.components_reference(comps[name])

    out, st = kept('ties top 1')
    assert out[0, 0, 20] == 1 and out[5, 17, 0] == 0 and st[4].tolist() == [3, 3, 1] and out[0, 19, 39] == 4
    out, st = kept('ties top 1 permuted')
    assert out[0, 5, 17] == 1 and out[20, 0, 0] == 0                                      # B: first in (i2, i0, i1) order
    out, st = kept('ties binary top 1')
    assert out[0, 0, 20] == 1 and out[5, 17, 0] == 0 and st[1].tolist() == [2, 24, 12]
    assert kept('ties per class')[1][1:].tolist() == [[2, 24, 12], [1, 12, 12], [2, 6, 6], [3, 3, 1]]
    out, st = kept('single voxels top 2')
    assert out[0, 19, 39] == 1 and out[8, 0, 39] == 1 and out[8, 19, 0] == 0 and st[1].tolist() == [3, 3, 2]
    out, st = kept('three blobs top 2')
    assert st[1].tolist() == [4, 73, 48] and out[3, 4, 15] == 1 and out[6, 10, 30] == 0     # the earlier of the two of 18
    assert kept('three blobs top 2 floor 19')[1][1].tolist() == [4, 73, 30]
    assert [kept('three blobs all floor %d' % f)[1][1, 2] for f in (17, 18, 19)] == [66, 66, 30]
    assert not kept('three blobs floor above all')[0].any() and not kept('three blobs floor 2^40')[0].any()
    assert kept('three blobs top 8')[1][1].tolist() == [4, 73, 73]
    assert kept('serpentine')[1][2].tolist() == [1, 3059, 3059]
    assert not kept('negative only')[0].any()


@pytest.mark.parametrize('index', range(len(HOLES)), ids=[c.name for c in HOLES])
def test_fill_holes_numpy_path_equals_flood_fill(index):
    from aide_amd.inference import fill_holes
    case = HOLES[index]
    for axis in case.axes:
        want, want_stats, _ = pc.holes_reference(index, axis)
        got, stats = fill_holes(case.volume, case.classes, axis, stats=True)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == case.volume.shape
        assert stats.dtype == np.int64 and stats.shape == (case.classes or 2, 2)
        assert np.array_equal(got, want), (case.name, axis, int((got != want).sum()))
        assert np.array_equal(stats, want_stats), (case.name, axis, stats, want_stats)
        assert np.array_equal(fill_holes(case.volume, case.classes, axis), got)
    assert np.array_equal(fill_holes(torch.from_numpy(case.volume.copy()), case.classes), pc.holes_reference(index, None)[0])


@pytest.mark.parametrize('index', [i for i, c in enumerate(HOLES) if c.classes is None],
                         ids=[c.name for c in HOLES if c.classes is None])
def test_fill_holes_binary_equals_scipy(index):
    from scipy import ndimage
    from aide_amd.inference import fill_holes
    vol = HOLES[index].volume
    assert np.array_equal(fill_holes(vol), ndimage.binary_fill_holes(vol != 0).astype(np.uint8))
    for axis in (0, 1, 2):
        want = np.stack([ndimage.binary_fill_holes(np.take(vol, j, axis=axis) != 0) for j in range(vol.shape[axis])], axis=axis)
        assert np.array_equal(fill_holes(vol, slice_axis=axis), want.astype(np.uint8)), axis


def test_fill_holes_two_classes_is_binary():
    from aide_amd.inference import fill_holes
    seen = 0
    for case in HOLES:
        if case.classes is None and set(np.unique(case.volume).tolist()) <= {0, 1}:
            seen += 1
            for axis in pc.AXES:
                got, stats = fill_holes(case.volume, 2, axis, stats=True)
                want, want_stats = fill_holes(case.volume, None, axis, stats=True)
                assert got.tobytes() == want.tobytes() and stats.tobytes() == want_stats.tobytes(), (case.name, axis)
    assert seen >= 10


@pytest.mark.parametrize('index', range(len(COMPONENTS)), ids=[c.name for c in COMPONENTS])
def test_keep_components_numpy_path_equals_flood_fill(index):
    from aide_amd.inference import keep_components
    case = COMPONENTS[index]
    want, want_stats = pc.components_reference(index)
    got = keep_components(case.volume, case.top_k, case.min_voxels, case.classes)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == case.volume.shape
    assert np.array_equal(got, want), (case.name, int((got != want).sum()))
    if case.classes is not None:
        again, stats = keep_components(case.volume, case.top_k, case.min_voxels, case.classes, stats=True)
        assert stats.dtype == np.int64 and stats.shape == (case.classes, 3)
        assert np.array_equal(again, want) and np.array_equal(stats, want_stats), (case.name, stats, want_stats)
    cpu = keep_components(torch.from_numpy(case.volume.copy()), case.top_k, case.min_voxels, case.classes)
    assert isinstance(cpu, np.ndarray) and np.array_equal(cpu, want)


def test_keep_components_defaults_are_the_existing_filters():
    from aide_amd.inference import keep_components, keep_largest_connected_components, keep_largest_per_class
    volumes = {}
    for case in COMPONENTS:
        volumes.setdefault(case.volume.tobytes() + repr(case.volume.shape).encode(), (case.name, case.volume))
    assert len(volumes) >= 20
    for name, vol in volumes.values():
        assert keep_components(vol).tobytes() == keep_largest_connected_components(vol).tobytes(), name
        assert keep_components(vol, 1, 1).tobytes() == keep_largest_connected_components(vol).tobytes(), name
        for c in (2, 5, 8):
            got, stats = keep_components(vol, 1, 1, c, stats=True)
            want, want_stats = keep_largest_per_class(vol, c, stats=True)
            assert got.tobytes() == want.tobytes() and stats.tobytes() == want_stats.tobytes(), (name, c)
            assert keep_components(vol, [1] * c, [1] * c, c).tobytes() == want.tobytes(), (name, c)


def test_python_argument_errors():
    from aide_amd.inference import keep_components, fill_holes, predict_case
    vol = np.zeros((2, 3, 4), np.int64)
    for bad in (dict(top_k=0), dict(top_k=9), dict(top_k=-1), dict(top_k=1.5), dict(top_k=True), dict(min_voxels=0),
                dict(min_voxels=-3), dict(min_voxels=None), dict(min_voxels=2.0), dict(num_classes=1), dict(num_classes=9),
                dict(num_classes=0), dict(top_k=(0, 1, 2)), dict(min_voxels=(1, 1)),
                dict(num_classes=3, top_k=(0, 1)), dict(num_classes=3, top_k=(0, 1, 2, 2)), dict(num_classes=3, min_voxels=(1, 1)),
                dict(num_classes=3, top_k=(0, 1, 9)), dict(num_classes=3, top_k=(0, 0, 1)), dict(num_classes=3, min_voxels=(1, 1, 0))):
        with pytest.raises(ValueError):
            keep_components(vol, **bad)
    assert not keep_components(vol, num_classes=3, top_k=(-5, 1, None), min_voxels=(0, 1, 7)).any()    # entry 0 is ignored
    with pytest.raises(TypeError):
        keep_components(vol, stats=True)
    for bad in (dict(num_classes=1), dict(num_classes=9), dict(slice_axis=3), dict(slice_axis=-1), dict(slice_axis=1.0)):
        with pytest.raises(ValueError):
            fill_holes(vol, **bad)
    with pytest.raises(TypeError):
        predict_case(None, None, top_k=2)
    with pytest.raises(TypeError):
        predict_case(None, None, min_voxels=5)
    with pytest.raises(TypeError):
        predict_case(None, None, slice_axis=2)
    with pytest.raises(TypeError):
        predict_case(None, None, keep_largest=True, num_classes=3, fill_holes=True)
    with pytest.raises(ValueError):
        predict_case(None, None, fill_holes='per_class')


def test_entry_points_declared_and_exported(built):
    from aide_amd._lib import lib, parse_header
    protos = parse_header()
    out = subprocess.run(['nm', '-D', '--defined-only', built], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW:
        assert name in protos and name in lib.protos and name in exported, name
    assert len(protos['aide_components3d_ws_bytes'][1]) == 1 and len(protos['aide_keep_components3d'][1]) == 14
    assert len(protos['aide_fill_holes3d_ws_bytes'][1]) == 1 and len(protos['aide_fill_holes3d'][1]) == 14


def test_workspace_queries(built):
    from aide_amd._lib import lib
    for query, per_voxel in ((lib.aide_components3d_ws_bytes, 8), (lib.aide_fill_holes3d_ws_bytes, 12)):
        assert query(2 ** 31) == 0 and query(-1) == 0 and query(2 ** 40) == 0
        sizes = [query(n) for n in (0, 1, 2, 255, 256, 257, 1000, 4096, 10 ** 6, 2 ** 31 - 1)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
        assert query(1000) >= per_voxel * 1000 + 16 and query(1000) % 4 == 0
        assert query(2 ** 31 - 1) >= per_voxel * (2 ** 31 - 1)


def test_entry_points_reject_without_launch(built):
    """answered on the host before any HIP call: every device pointer is null here"""
    from aide_amd._lib import lib
    ks, ms = (ctypes.c_int * 8)(0, 1, 1, 1, 1, 1, 1, 1), (ctypes.c_longlong * 8)(0, 1, 1, 1, 1, 1, 1, 1)
    keep = lib.aide_keep_components3d
    assert keep(None, 4, 4, 4, 16, 4, 1, 5, ks, ms, None, None, None, None) < 0              # null pointers
    assert keep(None, 4, 4, 4, 16, 4, 1, 0, ks, ms, None, None, None, None) < 0
    for c in (-1, 1, 9, 256):
        assert keep(None, 4, 4, 4, 16, 4, 1, c, ks, ms, None, None, None, None) < 0          # num_classes
        assert keep(None, 0, 4, 4, 16, 4, 1, c, ks, ms, None, None, None, None) < 0          # ... also for an empty volume
    assert keep(None, 4, 4, 4, 16, 4, 1, 5, None, ms, None, None, None, None) < 0            # no rule
    assert keep(None, 4, 4, 4, 16, 4, 1, 5, ks, None, None, None, None, None) < 0
    assert keep(None, 2 ** 16, 2 ** 15, 1, 2 ** 15, 1, 1, 5, ks, ms, None, None, None, None) < 0   # 2^31 voxels
    assert keep(None, -1, 4, 4, 16, 4, 1, 5, ks, ms, None, None, None, None) < 0
    assert keep(None, 0, 4, 4, 16, 4, 1, 5, ks, ms, None, None, None, None) == 0             # empty: nothing to do
    assert keep(None, 0, 4, 4, 16, 4, 1, 0, ks, ms, None, None, None, None) == 0
    for c, k, m in ((5, 9, 1), (5, -1, 1), (5, 1, 0), (5, 1, -7), (0, 9, 1), (0, 1, 0)):
        bad_k, bad_m = (ctypes.c_int * 8)(*ks), (ctypes.c_longlong * 8)(*ms)
        bad_k[1 if c == 0 else c - 1], bad_m[1 if c == 0 else c - 1] = k, m
        assert keep(None, 0, 4, 4, 16, 4, 1, c, bad_k, bad_m, None, None, None, None) < 0, (c, k, m)   # an entry out of range
    fill = lib.aide_fill_holes3d
    assert fill(None, 0, 4, 4, 4, 16, 4, 1, 5, -1, None, None, None, None) < 0               # null pointers
    assert fill(None, 1, 4, 4, 4, 16, 4, 1, 0, 2, None, None, None, None) < 0
    for c in (-1, 1, 9, 256):
        assert fill(None, 0, 0, 4, 4, 16, 4, 1, c, -1, None, None, None, None) < 0
    for axis in (-2, 3, 100):
        assert fill(None, 0, 0, 4, 4, 16, 4, 1, 5, axis, None, None, None, None) < 0
    for u8 in (-1, 2):
        assert fill(None, u8, 0, 4, 4, 16, 4, 1, 5, -1, None, None, None, None) < 0
    assert fill(None, 0, 2 ** 16, 2 ** 15, 1, 2 ** 15, 1, 1, 5, -1, None, None, None, None) < 0
    assert fill(None, 0, -1, 4, 4, 16, 4, 1, 5, -1, None, None, None, None) < 0
    assert fill(None, 0, 0, 4, 4, 16, 4, 1, 5, -1, None, None, None, None) == 0
    assert fill(None, 1, 4, 0, 4, 16, 4, 1, 0, 0, None, None, None, None) == 0
