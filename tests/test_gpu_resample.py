"""-m gpu: resampling on the device (aide_amd/csrc/resample3d.hip: aide_resample3d_labels / _image / _probs) against the host
statement of aide_amd/resample.py, byte for byte, on every geometry of resample_cases: every class count, both element types,
both orders; layouts; the tie rule; the same bytes whatever the table workspace held; `predict_case(target_spacing=)`; what the
entry points reject."""
import functools

import numpy as np
import pytest
import torch

import resample_cases as rc

pytestmark = pytest.mark.gpu

GEO = pytest.mark.parametrize('index', range(len(rc.GEOMETRIES)), ids=rc.IDS)
ERR_ARG = -1


@functools.lru_cache(maxsize=None)
def _host_labels(index, c, u8, order):
    from aide_amd.resample import resample_labels
    d, e = rc.GEOMETRIES[index]
    vol = rc.label_volume(d, c or 2, np.uint8 if u8 else np.int64)
    want = resample_labels(vol, e, c, order=order)
    want.setflags(write=False)
    return vol, want


@GEO
def test_labels_equal_the_host_statement(dev, index):
    from aide_amd.resample import resample_labels
    e = rc.GEOMETRIES[index][1]
    for c in (None, 2, 3, 4, 5, 6, 7, 8):
        for u8 in (False, True):
            for order in (1, 0):
                vol, want = _host_labels(index, c, u8, order)
                t = torch.from_numpy(vol).to(dev)
                got = resample_labels(t, e, c, order=order)
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == e and got.is_contiguous()
                assert np.array_equal(got.cpu().numpy(), want), (c, u8, order)
                assert np.array_equal(t.cpu().numpy(), vol)                      # the input is unchanged


@GEO
def test_image_bits_equal_the_host_statement(dev, index):
    from aide_amd.resample import resample_image
    d, e = rc.GEOMETRIES[index]
    x = np.stack([rc.image(d), rc.image(d, 1), rc.image(d, 2)]).reshape((3, 1) + d)
    special = x[2, 0].reshape(-1)[::5]                                        # (a view: the third volume holds non-finite values)
    special[:] = np.resize(np.array([np.inf, -np.inf, np.nan, -0.0, 1e-42], np.float32), special.shape)
    t = torch.from_numpy(x).to(dev)
    for order in (1, 0):
        with np.errstate(invalid='ignore'):
            want = resample_image(x, e, order=order)
        got = resample_image(t, e, order=order)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 1) + e
        got = got.cpu().numpy()
        assert got[:2].tobytes() == want[:2].tobytes(), order
        nan = np.isnan(want[2])                                               # a NaN is a NaN: its sign and payload are not part of the contract
        assert np.array_equal(np.isnan(got[2]), nan) and got[2][~nan].tobytes() == want[2][~nan].tobytes(), order
        assert resample_image(t[1, 0], e, order=order).cpu().numpy().tobytes() == want[1, 0].tobytes()
    assert t.cpu().numpy().tobytes() == x.tobytes()


@GEO
def test_probs_equal_the_host_statement(dev, index):
    from aide_amd.resample import resample_probs
    d, e = rc.GEOMETRIES[index]
    for c in range(2, 9):
        p = rc.probabilities(d, c)
        t = torch.from_numpy(p).to(dev)
        want_labels, want_probs = resample_probs(p, e, probs_out=True)
        labels, probs = resample_probs(t, e, probs_out=True)
        assert labels.dtype == torch.int64 and tuple(labels.shape) == e and tuple(probs.shape) == (e[0], c) + e[1:]
        assert np.array_equal(labels.cpu().numpy(), want_labels), c
        assert probs.cpu().numpy().tobytes() == want_probs.tobytes(), c
        assert torch.equal(resample_probs(t, e), labels)
        assert t.cpu().numpy().tobytes() == p.tobytes()


@pytest.mark.parametrize('index', (0, 2, 8), ids=[rc.IDS[i] for i in (0, 2, 8)])
def test_layouts(dev, index):
    """a permuted [H,W,S] view, a sliced view and a contiguous copy give the same bytes; the result of a permuted view lies in
    the memory order of its source; [S,C,H,W] probabilities and image batches are read where they lie"""
    from aide_amd.resample import resample_image, resample_labels, resample_probs
    d, e = rc.GEOMETRIES[index]
    for u8 in (False, True):
        vol, want = _host_labels(index, 5, u8, 1)
        t = torch.from_numpy(vol).to(dev)
        shw = t.permute(2, 0, 1).contiguous()                                   # memory [S,H,W], viewed as [H,W,S]
        view = shw.permute(1, 2, 0)
        assert not view.is_contiguous() and torch.equal(view, t)
        got = resample_labels(view, e, 5)
        assert np.array_equal(got.cpu().numpy(), want)
        assert got.permute(2, 0, 1).is_contiguous() or 1 in e
        big = torch.full((2 * d[0] + 1, d[1] + 3, 3 * d[2] + 2), 4, device=dev, dtype=t.dtype)
        sliced = big[1::2, 2:2 + d[1], 1::3][:d[0], :, :d[2]]
        sliced.copy_(t)
        assert not sliced.is_contiguous() or t.numel() == 1
        for order in (1, 0):
            want_o = _host_labels(index, 5, u8, order)[1]
            assert np.array_equal(resample_labels(sliced, e, 5, order=order).cpu().numpy(), want_o)
            assert np.array_equal(resample_labels(view, e, 5, order=order).cpu().numpy(), want_o)
    p = rc.probabilities(d, 3)
    big = torch.zeros((d[0] + 2, 6, 2 * d[1], d[2] + 5), device=dev)
    view = big[1:1 + d[0], 2:5, ::2, 3:3 + d[2]]
    view.copy_(torch.from_numpy(p))
    assert not view.is_contiguous()
    want_labels, want_probs = resample_probs(p, e, probs_out=True)
    labels, probs = resample_probs(view, e, probs_out=True)
    assert np.array_equal(labels.cpu().numpy(), want_labels) and probs.cpu().numpy().tobytes() == want_probs.tobytes()
    x = np.stack([rc.image(d), rc.image(d, 1)])
    wide = torch.zeros((2,) + d[:2] + (d[2] + 3,), device=dev)
    wide[..., 1:1 + d[2]] = torch.from_numpy(x).to(dev)
    assert resample_image(wide[..., 1:1 + d[2]], e).cpu().numpy().tobytes() == resample_image(x, e).tobytes()


def test_tie_rule(dev):
    """the halving geometry against the block-majority rule; two equal classes everywhere give the lower index"""
    from aide_amd.resample import resample_labels, resample_probs
    d, e = rc.GEOMETRIES[rc.HALVING]
    for c in (None,) + rc.CLASSES:
        for dtype in (np.int64, np.uint8):
            vol = rc.label_volume(d, c or 2, dtype)
            got = resample_labels(torch.from_numpy(vol).to(dev), e, c).cpu().numpy()
            assert np.array_equal(got, rc.block_majority(vol.astype(np.int64) if c else (vol != 0).astype(np.int64), c or 2)), (c, dtype)
    for gd, ge in rc.GEOMETRIES:
        p = rc.probabilities(gd, 5)
        p[:, 3] = p[:, 1]
        p[:, 4] = p[:, 0]
        labels = resample_probs(torch.from_numpy(p).to(dev), ge).cpu().numpy()
        assert not (labels >= 3).any() and np.array_equal(labels, resample_probs(p, ge))
    same = torch.full((3, 4, 5, 6), 0.25, device=dev)
    assert not resample_probs(same, (5, 7, 4)).any()


def test_same_bytes_whatever_the_workspace_held(dev):
    """two calls through the entry points on one workspace, filled with 0xFF in between"""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    for index in (0, 1, 8):
        d, e = rc.GEOMETRIES[index]
        ws = torch.zeros(lib.aide_resample3d_ws_bytes(*e), device=dev, dtype=torch.uint8)
        assert ws.numel() == 16 * sum(e)
        vol, want = _host_labels(index, 5, False, 1)
        t = torch.from_numpy(vol).to(dev)
        p = torch.from_numpy(rc.probabilities(d, 4)).to(dev)
        x = torch.from_numpy(rc.image(d)).to(dev)
        runs = []
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            out = torch.full(e, 9, device=dev, dtype=torch.uint8)
            check(lib.aide_resample3d_labels(ptr(t), 0, *d, *t.stride(), *e, 5, 1, 0, 1, 2, ptr(out), ptr(ws), stream_ptr()), 'labels')
            ws.fill_(fill)
            labels = torch.full(e, -1, device=dev, dtype=torch.int64)
            probs = torch.full((e[0], 4) + e[1:], -1.0, device=dev)
            check(lib.aide_resample3d_probs(ptr(p), 4, p.stride(1), *d, p.stride(0), p.stride(2), p.stride(3), *e, ptr(labels),
                                            ptr(probs), ptr(ws), stream_ptr()), 'probs')
            ws.fill_(fill)
            y = torch.full(e, -1.0, device=dev)
            check(lib.aide_resample3d_image(ptr(x), 1, 0, *d, *x.stride(), *e, 1, ptr(y), ptr(ws), stream_ptr()), 'image')
            runs.append(tuple(r.cpu().numpy().tobytes() for r in (out, labels, probs, y)))
            assert np.array_equal(out.cpu().numpy(), want)
        assert runs[0] == runs[1], rc.IDS[index]


def test_two_launches_per_call(dev):
    from aide_amd.profiling import DispatchTimer
    from aide_amd.resample import resample_image, resample_labels, resample_probs

    def launches(call):
        torch.cuda.synchronize()
        timer = DispatchTimer(16, families=[15])
        timer.start()
        try:
            call()
        finally:
            timer.stop()
        return len(timer.timeline())

    d, e = rc.GEOMETRIES[8]
    t = torch.from_numpy(rc.label_volume(d, 5)).to(dev)
    p = torch.from_numpy(rc.probabilities(d, 8)).to(dev)
    x = torch.from_numpy(rc.image(d)).to(dev)
    for order in (0, 1):
        assert launches(lambda: resample_labels(t, e, 5, order=order)) == 2
        assert launches(lambda: resample_image(x, e, order=order)) == 2
    assert launches(lambda: resample_probs(p, e, probs_out=True)) == 2


@pytest.fixture(scope='module')
def tiny_net(dev):
    """the narrowest UNet with three classes, in eval mode: the first seed whose network (two channels feed its head) gives
    at least two classes a twentieth of a probe each, so that the comparisons below are not between constant volumes"""
    from aide_amd.inference import predict_labels
    from aide_amd.models_singlemodalinput import UNet2
    g = torch.Generator().manual_seed(3)
    probe = torch.randn(4, 3, 48, 32, generator=g).to(dev)
    for seed in range(11, 43):
        torch.manual_seed(seed)
        net = UNet2(3)
        with torch.no_grad():
            net.last_conv1.weight.normal_(0.0, 1.0)
            net.last_conv1.bias.zero_()
        net = net.to(dev)
        net.train()
        with torch.no_grad():
            for _ in range(2):
                net(torch.randn(4, 3, 32, 32, generator=g).to(dev))
        net.eval()
        share = torch.bincount(predict_labels(net, probe, batch_size=4).reshape(-1), minlength=3).float() / probe[:, 0].numel()
        if int((share > 0.05).sum()) >= 2:
            return net, g
    raise AssertionError('no seed in 11 .. 42 gives a network that predicts more than one class')


def test_predict_case_target_spacing(dev, tiny_net):
    """4 slices of 24 x 40 at spacing (2, 1, 5) with target_spacing (1, 1): the 48 x 40 grid is no multiple of 16, so the call
    needs window= (and says so without it); 24 x 32 slices give 48 x 32 and take the plain path.  Either way the result is the
    composition resample_image -> predict_case(probs=True) on the resampled input -> resample_probs, written out here."""
    from aide_amd.inference import predict_case, keep_largest_per_class, resample_image, resample_probs, resampled_shape
    net, g = tiny_net
    sp, target = (2.0, 1.0, 5.0), (1.0, 1.0)
    for (h, w), extra in (((24, 40), dict(window=32)), ((24, 32), {})):
        slices = torch.randn(4, 3, h, w, generator=g).to(dev)
        (hn, wn, sn), real = resampled_shape((h, w, 4), sp, target + sp[2:])
        assert (hn, wn, sn) == (48, w, 4) and real == (1.0, 1.0, 5.0)
        fine = resample_image(slices.reshape(12, 1, h, w), (1, hn, wn)).reshape(4, 3, hn, wn)
        for views in (None, 'flip2'):
            kw = dict(extra, batch_size=4, numpy=False, views=views)
            _, pr = predict_case(net, fine, probs=True, **kw)
            assert tuple(pr.shape) == (4, 3, hn, wn)
            labels, back = resample_probs(pr, (4, h, w), probs_out=True)
            want = labels.permute(1, 2, 0)
            got = predict_case(net, slices, spacing=sp, target_spacing=target, **kw)
            assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (h, w, 4) and torch.equal(got, want)
            assert len(torch.unique(got)) > 1
            got, probs = predict_case(net, slices, spacing=sp, target_spacing=target, probs=True, **kw)
            assert torch.equal(got, want) and torch.equal(probs, back)
            got = predict_case(net, slices, spacing=sp, target_spacing=target, keep_largest='per_class', num_classes=3, **kw)
            assert got.dtype == torch.uint8 and torch.equal(got, keep_largest_per_class(want, 3))
        host = predict_case(net, slices, spacing=sp, target_spacing=target, batch_size=4, **extra)
        assert isinstance(host, np.ndarray) and np.array_equal(host, predict_case(net, slices, spacing=sp, target_spacing=target,
                                                                                  batch_size=4, numpy=False, **extra).cpu().numpy())
    slices = torch.randn(4, 3, 24, 40, generator=g).to(dev)
    with pytest.raises(ValueError, match='window='):
        predict_case(net, slices, spacing=sp, target_spacing=target)
    with pytest.raises(TypeError):
        predict_case(net, slices, target_spacing=target)
    with pytest.raises(TypeError):
        predict_case(net, slices, spacing=sp)
    with pytest.raises(ValueError):
        predict_case(net, slices, spacing=sp, target_spacing=(1.0, 0.0))
    with pytest.raises(ValueError):
        predict_case(net, slices, spacing=sp, target_spacing=(1.0, 1.0, 5.0))
    square = torch.randn(4, 3, 32, 32, generator=g).to(dev)                    # equal shapes: the path the call took before
    plain = predict_case(net, square, batch_size=4, numpy=False)
    same = predict_case(net, square, batch_size=4, numpy=False, spacing=(1.0, 1.004, 5.0), target_spacing=(1.0, 1.0))
    assert torch.equal(same, plain) and same.stride() == plain.stride() and same.dtype == plain.dtype


def test_entry_points_reject_before_any_launch(dev):
    """AIDE_ERR_ARG for every argument the header lists, with nothing written"""
    from aide_amd._lib import lib
    from aide_amd.ops import ptr, stream_ptr
    d, e = (3, 4, 5), (4, 6, 8)
    v = torch.zeros(d, device=dev, dtype=torch.int64)
    x = torch.zeros(d, device=dev)
    p = torch.zeros((3, 2, 4, 5), device=dev)
    out = torch.full((4 * 6 * 8 + 16,), 7, device=dev, dtype=torch.uint8)
    y = torch.full((4 * 6 * 8 + 4,), 7.0, device=dev)
    labels = torch.full((4 * 6 * 8 + 2,), 7, device=dev, dtype=torch.int64)
    probs = torch.full((2 * 4 * 6 * 8 + 4,), 7.0, device=dev)
    ws = torch.zeros(lib.aide_resample3d_ws_bytes(*e) + 16, device=dev, dtype=torch.uint8)
    big = (2 ** 11, 2 ** 10, 2 ** 10)
    assert lib.aide_resample3d_ws_bytes(*big) == 0 and lib.aide_resample3d_ws_bytes(-1, 1, 1) == 0

    def lab(v_ptr=ptr(v), u8=0, d=d, s=v.stride(), e=e, c=2, order=1, oa=(0, 1, 2), o=ptr(out), w=ptr(ws)):
        return lib.aide_resample3d_labels(v_ptr, u8, *d, *s, *e, c, order, *oa, o, w, stream_ptr())

    def img(x_ptr=ptr(x), batch=1, d=d, e=e, order=1, o=ptr(y), w=ptr(ws)):
        return lib.aide_resample3d_image(x_ptr, batch, 0, *d, *x.stride(), *e, order, o, w, stream_ptr())

    def prb(p_ptr=ptr(p), c=2, d=d, e=e, lb=ptr(labels), po=ptr(probs), w=ptr(ws)):
        return lib.aide_resample3d_probs(p_ptr, c, p.stride(1), *d, p.stride(0), p.stride(2), p.stride(3), *e, lb, po, w, stream_ptr())

    off = lambda t, n: type(ptr(t))(t.data_ptr() + n)
    for call in (lab, img, prb):
        assert call(d=(-1, 4, 5)) == ERR_ARG and call(e=(4, -6, 8)) == ERR_ARG
        assert call(d=big) == ERR_ARG and call(e=big) == ERR_ARG
        assert call(d=(0, 4, 5)) == ERR_ARG                                     # an empty input for an output that is not
        assert call(w=None) == ERR_ARG and call(w=off(ws, 8)) == ERR_ARG
        assert call(e=(4, 0, 8), w=None) == 0                                   # an empty output: nothing to do, nothing looked at
    for call in (lab, img):
        assert call(order=2) == ERR_ARG and call(order=-1) == ERR_ARG
    assert lab(u8=2) == ERR_ARG and lab(c=1) == ERR_ARG and lab(c=9) == ERR_ARG and lab(c=-2) == ERR_ARG
    assert lab(oa=(0, 1, 1)) == ERR_ARG and lab(oa=(0, 1, 3)) == ERR_ARG and lab(oa=(-1, 1, 2)) == ERR_ARG
    assert lab(v_ptr=None) == ERR_ARG and lab(o=None) == ERR_ARG and lab(o=off(out, 2)) == ERR_ARG and lab(v_ptr=off(v, 4)) == ERR_ARG
    assert img(batch=-1) == ERR_ARG and img(batch=2 ** 24) == ERR_ARG            # 2^24 * 192 voxels
    assert img(x_ptr=None) == ERR_ARG and img(o=None) == ERR_ARG and img(x_ptr=off(x, 2)) == ERR_ARG and img(o=off(y, 4)) == ERR_ARG
    assert prb(c=1) == ERR_ARG and prb(c=9) == ERR_ARG and prb(c=8, e=(2 ** 10, 2 ** 10, 2 ** 9)) == ERR_ARG
    assert prb(p_ptr=None) == ERR_ARG and prb(lb=None) == ERR_ARG and prb(p_ptr=off(p, 2)) == ERR_ARG
    assert prb(lb=off(labels, 8)) == ERR_ARG and prb(po=off(probs, 4)) == ERR_ARG
    assert img(batch=0, w=None) == 0
    torch.cuda.synchronize()
    assert (out == 7).all() and (y == 7.0).all() and (labels == 7).all() and (probs == 7.0).all() and not ws.any()
    assert lab() == 0 and img() == 0 and prb() == 0 and prb(po=None) == 0          # ... and the same calls with good arguments run
    torch.cuda.synchronize()
    assert not out[:192].any() and (out[192:] == 7).all() and not y[:192].any() and (y[192:] == 7.0).all()
    assert not labels[:192].any() and (labels[192:] == 7).all() and not probs[:384].any() and (probs[384:] == 7.0).all()
