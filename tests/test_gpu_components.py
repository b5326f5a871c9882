"""-m gpu: the labelled components and the lesion-wise counts on the device (aide_amd/csrc/eval3d.hip, aide_label_components3d
and aide_lesion_counts3d) equal the flood fill of components_cases byte for byte on every case; every call is issued twice and
must give the same bytes; the input is left as it was.  Everything is integer."""
import numpy as np
import pytest
import torch

import components_cases as cc

pytestmark = pytest.mark.gpu

LABELS = cc.label_cases()
PAIRS = cc.pair_cases()
TORCH = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


def _device(vol, dev):
    t = torch.from_numpy(np.array(vol, order='K', copy=True)).to(dev)
    if vol.flags['C_CONTIGUOUS']:
        assert t.is_contiguous()
    else:                                         # a view stays a view: the kernels get its strides
        assert t.stride() == tuple(s // vol.itemsize for s in vol.strides) and not t.is_contiguous()
    return t


def _label_twice(t, classes, cap=65536):
    """(labels, count, props) of a device call as numpy arrays, after a second call gave the same bytes"""
    from aide_amd.inference import label_components
    runs = []
    for _ in range(2):
        labels, count, props = label_components(t, classes, props=True, max_blobs=cap)
        assert labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape == t.shape
        assert count.is_cuda and count.dtype == torch.int64 and tuple(count.shape) == (1,)
        assert props.is_cuda and props.dtype == torch.int64 and tuple(props.shape) == (cap, 12)
        runs.append((labels.cpu().numpy(), count.cpu().numpy(), props.cpu().numpy()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    return runs[0]


@pytest.mark.parametrize('index', range(len(LABELS)), ids=[c.name for c in LABELS])
def test_label_components_device_equals_flood_fill(dev, index):
    from aide_amd.inference import label_components
    case = LABELS[index]
    t = _device(case.volume, dev)
    assert t.dtype == TORCH[case.volume.dtype]
    before = t.clone()
    want, want_count, want_props = cc.label_reference(index)
    labels, count, props = _label_twice(t, case.classes)
    assert int(count[0]) == want_count, (case.name, count, want_count)
    assert labels.tobytes() == want.tobytes(), (case.name, int((labels != want).sum()))
    assert props.tobytes() == want_props.tobytes(), (case.name, np.argwhere(props != want_props)[:8])
    alone = label_components(t, case.classes)                                             # the write without the props table
    assert len(alone) == 2 and alone[0].cpu().numpy().tobytes() == want.tobytes() and int(alone[1].cpu()[0]) == want_count
    assert torch.equal(t, before) and t.stride() == before.stride()


def test_cap_below_the_count(dev):
    from aide_amd.inference import region_table
    vol = cc.three_blobs()
    t = _device(vol, dev)
    want, want_count, want_props = cc.flood_labels(vol, None, 2)
    assert want_count == 4
    labels, count, props = _label_twice(t, None, 2)
    assert int(count[0]) == 4 and labels.tobytes() == want.tobytes() and props.tobytes() == want_props.tobytes()
    assert (props[:, 1] == [30, 18]).all()
    labels, count, props = _label_twice(t, None, 7)                                       # rows from count on are zero
    assert props.tobytes() == cc.flood_labels(vol, None, 7)[2].tobytes() and not props[4:].any() and props[:4, 1].all()
    from aide_amd.inference import label_components
    _, count, props = label_components(t, None, props=True, max_blobs=7)
    table = region_table(props, count)
    assert table['count'] == 4 and table['area'].tolist() == [30, 18, 18, 7]
    assert np.array_equal(table['centroid'][0], np.argwhere(vol[:2, :3, :5] == 1).mean(axis=0))


def test_labels_agree_with_the_device_filters(dev):
    """labels != 0 is keep_components(top_k=None); 1 + the first maximum of the props areas is the blob that
    keep_largest_connected_components keeps: wherever the volume has a positive voxel"""
    from aide_amd.inference import label_components, keep_components, keep_largest_connected_components
    seen = 0
    for case in LABELS:
        if case.classes is not None or not (case.volume.size and case.volume.max() > 0):
            continue
        t = _device(case.volume, dev)
        labels, count, props = label_components(t, props=True)
        assert torch.equal((labels != 0).to(torch.uint8), keep_components(t, top_k=None)), case.name
        n = int(count.cpu()[0])
        assert 1 <= n <= 65536
        best = 1 + int(np.argmax(props[:n, 1].cpu().numpy()))                             # numpy: the first maximum
        assert torch.equal((labels == best).to(torch.uint8), keep_largest_connected_components(t)), case.name
        seen += 1
    assert seen >= 30


@pytest.mark.parametrize('index', range(len(PAIRS)), ids=[c.name for c in PAIRS])
def test_lesion_counts_device_equal_flood_fill(dev, index):
    from aide_amd.inference import lesion_counts, lesion_scores, case_scores
    case = PAIRS[index]
    p, t = _device(case.pred, dev), _device(case.target, dev)
    before = p.clone(), t.clone()
    sides = cc.pair_reference(index)
    for overlap in cc.OVERLAPS:
        want = cc.flood_lesions(sides, case.classes, overlap)
        runs = []
        for _ in range(2):
            got = lesion_counts(p, t, case.classes, overlap)
            assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (case.classes or 2, 6)
            runs.append(got.cpu().numpy())
        assert runs[0].tobytes() == runs[1].tobytes()
        assert runs[0].tobytes() == want.tobytes(), (case.name, overlap, runs[0], want)
        scores, want_scores = lesion_scores(p, t, case.classes, overlap), cc.scores_of(want, case.classes)
        assert tuple(scores) == tuple(want_scores)
        for key in scores:
            assert np.array_equal(np.asarray(scores[key]), np.asarray(want_scores[key]), equal_nan=True), (case.name, overlap, key)
    if case.classes is None:                      # column 5 is the voxel-wise TP of the device's case_scores
        tp = case_scores((p != 0).to(torch.int64), (t != 0).to(torch.int64))['TP']
        assert want[1, 4] == tp
    else:
        tp = case_scores(p, t, case.classes)['TP']
        assert np.array_equal(want[1:, 4], tp[1:])
    assert torch.equal(p, before[0]) and torch.equal(t, before[1])
    assert p.stride() == before[0].stride() and t.stride() == before[1].stride()


def test_case_scores_with_lesions_on_the_device(dev):
    from aide_amd.inference import case_scores, lesion_scores
    case = {c.name: c for c in PAIRS}['random classes 9x40x21 0.6']
    p, t = _device(case.pred, dev), _device(case.target, dev)
    old = case_scores(p, t, 5)
    new = case_scores(p, t, 5, lesions=0.5)
    host = case_scores(case.pred, case.target, 5, lesions=0.5)
    assert tuple(old) == ('Dice', 'IoU', 'TP', 'TN', 'FP', 'FN') and tuple(new) == tuple(host) and len(new) == 15
    for key in new:
        assert np.array_equal(new[key], host[key], equal_nan=True), key
    mixed = lesion_scores(case.pred, t, 5, 0.5)   # a host array against a device tensor goes to the device
    assert np.array_equal(mixed['detected'], host['lesion_detected'])


def test_same_bytes_whatever_the_workspace_held(dev):
    """through the C ABI on one workspace filled with 0x00 and with 0xFF before the call: stale control words, parents, areas,
    ranks, block counts or cover words would show (a fresh torch.empty may happen to be clean)"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    names = {case.name: index for index, case in enumerate(LABELS)}
    for name in ('serpentine 9x33x35 C=5', 'eight classes 9x40x21 binary', 'ties top 1 permuted 40x9x20 C=5'):
        index = names[name]
        case = LABELS[index]
        want, want_count, want_props = cc.label_reference(index)
        t = _device(case.volume, dev)
        ws = torch.empty(lib.aide_label_components3d_ws_bytes(t.numel()), device=dev, dtype=torch.uint8)
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            labels = torch.full(t.shape, -7, device=dev, dtype=torch.int32)
            count = torch.full((1,), -1, device=dev, dtype=torch.int64)
            props = torch.full((want_count + 3, 12), -1, device=dev, dtype=torch.int64)
            check(lib.aide_label_components3d(ptr(t), *t.shape, *t.stride(), case.classes or 0, ptr(labels), ptr(count),
                                              ptr(props), want_count + 3, ptr(ws), stream_ptr()), 'label_components3d')
            assert labels.cpu().numpy().tobytes() == want.tobytes() and int(count.cpu()[0]) == want_count, (name, fill)
            assert props.cpu().numpy().tobytes() == want_props[:want_count + 3].tobytes(), (name, fill)
    names = {case.name: index for index, case in enumerate(PAIRS)}
    for name in ('hand C=5', 'random binary 9x40x21 0.8'):
        index = names[name]
        case = PAIRS[index]
        want = cc.flood_lesions(cc.pair_reference(index), case.classes, 0.5)
        p, t = _device(case.pred, dev), _device(case.target, dev)
        ws = torch.empty(lib.aide_lesion_counts3d_ws_bytes(t.numel()), device=dev, dtype=torch.uint8)
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            out = torch.full((case.classes or 2, 6), -1, device=dev, dtype=torch.int64)
            check(lib.aide_lesion_counts3d(ptr(p), *p.stride(), ptr(t), *t.stride(), *p.shape, case.classes or 0, 0.5, ptr(out),
                                           ptr(ws), stream_ptr()), 'lesion_counts3d')
            assert out.cpu().numpy().tobytes() == want.tobytes(), (name, fill, out.tolist())


def test_launch_counts(dev):
    """the kernel timer counts the launches themselves: seven for label_components and ten for lesion_counts whatever the
    volume, the class count, the cap and props are"""
    from aide_amd.profiling import DispatchTimer
    from aide_amd.inference import label_components, lesion_counts

    def launches(call):
        torch.cuda.synchronize()
        timer = DispatchTimer(32, families=[15])  # family 15: the kernels of eval3d.hip (and other small ones)
        timer.start()
        try:
            call()
        finally:
            timer.stop()
        return len(timer.timeline())

    names = {case.name: case for case in LABELS}
    for name in ('all zero 5x17x33 binary', 'eight classes 9x40x21 binary', 'tiny 1x1x1 1x1x1 binary', 'serpentine 9x33x35 binary'):
        t = _device(names[name].volume, dev)
        for c in (None, 2, 8):
            assert launches(lambda: label_components(t, c)) == 7, (name, c)
            assert launches(lambda: label_components(t, c, props=True, max_blobs=5)) == 7, (name, c)
            assert launches(lambda: lesion_counts(t, t, c, 0.5)) == 10, (name, c)


def test_empty_volume(dev):
    from aide_amd.inference import label_components, lesion_counts
    empty = torch.zeros(0, 4, 4, dtype=torch.int64, device=dev)
    labels, count, props = label_components(empty, 5, props=True, max_blobs=3)
    assert labels.numel() == 0 and labels.dtype == torch.int32 and count.cpu().tolist() == [0] and not props.cpu().numpy().any()
    assert tuple(props.shape) == (3, 12)
    assert not lesion_counts(empty, empty, 5, 0.5).cpu().numpy().any()


def test_past_the_scan_boundaries(dev):
    """(34, 250, 250), no multiple of the tile: 2 125 000 nodes = 2076 blocks of 1024 nodes in the rank launches, so the one
    workgroup that scans the block counts (1024 per trip) makes three trips and carries its running total twice: the scan's
    second level is crossed at this size, no larger one is needed.  265 626 blobs: above the default cap and above 2^16.  Checked
    against the host statement (test_components_host.py holds that to the flood fill; the pure-Python flood fill is too slow
    here): labels and count complete, the first 65 536 props rows exact, and lesion_counts against a copy shifted by one voxel
    along i2."""
    from aide_amd.inference import label_components, lesion_counts
    vol = cc.lattice_case()
    assert vol.shape == (34, 250, 250) and (vol.size + 1023) // 1024 > 2 * 1024
    t = torch.from_numpy(vol).to(dev)
    want, want_count, want_props = label_components(vol, 5, props=True)
    assert int(want_count[0]) == 17 * 125 * 125 + 1 > 65536 and want_props[-1, 1] == 1
    assert want_props[:, 1].max() > 250 * 125 * 17                                        # the serpentine is among the first rows
    labels, count, props = label_components(t, 5, props=True)
    assert int(count.cpu()[0]) == int(want_count[0])
    assert labels.cpu().numpy().tobytes() == want.tobytes()
    assert props.cpu().numpy().tobytes() == want_props.tobytes()
    labels, count = label_components(t)           # the binary form: the same blobs, every value a member
    assert int(count.cpu()[0]) == int(want_count[0]) and labels.cpu().numpy().tobytes() == want.tobytes()
    shifted = np.zeros_like(vol)
    shifted[:, :, 1:] = vol[:, :, :-1]
    s = torch.from_numpy(shifted).to(dev)
    for c, overlap in ((5, 0.5), (None, 0.1)):
        got = lesion_counts(s, t, c, overlap).cpu().numpy()
        host = lesion_counts(shifted, vol, c, overlap)
        assert host[:, 0].sum() == int(want_count[0]) and host[:, 1].sum() == 1             # the serpentine meets itself
        assert got.tobytes() == host.tobytes(), (c, overlap, got, host)
