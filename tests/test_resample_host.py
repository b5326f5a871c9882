"""The host statement of aide_amd/resample.py (numpy float64, the definition the kernels are held to) against references that do
not come from it: scipy.ndimage.zoom(mode='nearest', grid_mode=True) for images, for the arg-max of the zoomed one-hot planes
and for order 0; the block-majority rule on the halving geometry; identities; `resampled_shape`; the argument errors."""
import numpy as np
import pytest
import torch

import resample_cases as rc
from aide_amd.resample import _interp, resample_image, resample_labels, resample_probs, resampled_shape

GEO = pytest.mark.parametrize('index', range(len(rc.GEOMETRIES)), ids=rc.IDS)


@GEO
def test_image_against_scipy(index):
    """Both sides evaluate sum w_i x_i over the same eight voxels with weights that are products of per-axis (1 - t, t), in
    float64 (u = 2^-53).  scipy forms the coordinate (o + 0.5) * (n_in / n_out) - 0.5 in floating point: a rounded quotient, a
    rounded product and a rounded difference of numbers below n_in + 1, an absolute error of the fraction t of at most
    3 u n_in; a change dt of t moves the interpolant along that axis by dt |x_hi - x_lo| <= 2 dt max|x|, so the three axes
    give 18 u n_max max|x|.  The statement's own t is one correctly rounded quotient; its weights, products and seven sums,
    and scipy's, add less than 16 u max|x| each.  Bound between the float64 values: (18 n_max + 32) u max|x|; the float32
    result is the rounded float64 sum, which adds 2^-24 |want|.  (Measured on these geometries: at most 5.6e-15 max|x|.)"""
    d, e = rc.GEOMETRIES[index]
    x = rc.image(d)
    want = rc.zoom(x.astype(np.float64), e)
    got = resample_image(x, e)
    assert got.dtype == np.float32 and got.shape == e
    acc = _interp(x.astype(np.float64), e)                                  # the float64 sums before the one rounding
    assert got.tobytes() == acc.astype(np.float32).tobytes()
    bound = (18 * max(d) + 32) * 2.0 ** -53 * np.abs(x).max()
    print('max float64 err / max|x| = %.3g, bound %.3g' % (np.abs(acc - want).max() / np.abs(x).max(), bound / np.abs(x).max()))
    assert (np.abs(acc - want) <= bound).all()
    assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + bound).all()
    batch = np.stack([x, rc.image(d, 1)]).reshape((2, 1) + d)              # leading dims are a batch
    both = resample_image(batch, e)
    assert both.shape == (2, 1) + e and both[0, 0].tobytes() == got.tobytes()
    assert both[1, 0].tobytes() == resample_image(rc.image(d, 1), e).tobytes()


@GEO
@pytest.mark.parametrize('c', rc.CLASSES)
def test_labels_against_scipy(index, c):
    """equal to the arg-max of the c zoomed one-hot planes wherever scipy's best class sum beats the second by more than 1e-9;
    on the generic and x 2 geometries that margin may exclude at most 2 % of the voxels (a condition on the inputs, asserted
    from the reference alone)"""
    d, e = rc.GEOMETRIES[index]
    vol = rc.label_volume(d, c)
    assert vol.size <= 4 or ((vol >= c).any() and (vol < 0).any())
    want, decided = rc.scipy_labels(vol, e, c)
    print('undecided: %.2f %%' % (100.0 * (~decided).mean()))
    if index in rc.CAPPED:
        assert (~decided).mean() <= 0.02
    got = resample_labels(vol, e, c)
    assert got.dtype == np.uint8 and got.shape == e
    assert np.array_equal(got[decided], want[decided])
    assert np.array_equal(resample_labels(torch.from_numpy(vol), e, c), got)                  # a CPU tensor takes the same path
    vol8 = rc.label_volume(d, c, np.uint8)
    assert np.array_equal(resample_labels(vol8, e, c), resample_labels(vol8.astype(np.int64), e, c))


@pytest.mark.parametrize('c', (None,) + rc.CLASSES)
def test_halving_is_the_block_majority(c):
    d, e = rc.GEOMETRIES[rc.HALVING]
    vol = rc.label_volume(d, c or 2)
    got = resample_labels(vol, e, c)
    assert np.array_equal(got, rc.block_majority(vol if c else (vol != 0).astype(np.int64), c or 2))
    assert len(np.unique(got)) > 1


@GEO
def test_order0_equals_scipy(index):
    d, e = rc.GEOMETRIES[index]
    x = rc.image(d)
    assert np.array_equal(resample_image(x, e, order=0), rc.zoom(x, e, order=0))
    for c in rc.CLASSES:
        vol = rc.label_volume(d, c)
        want = rc.zoom(vol, e, order=0)
        assert np.array_equal(resample_labels(vol, e, c, order=0), np.where((want >= 0) & (want < c), want, 0))
        assert np.array_equal(resample_labels(vol, e, None, order=0), want != 0)


def test_identity_returns_the_input():
    d = (3, 4, 5)
    x = rc.image(d)
    for order in (0, 1):
        assert resample_image(x, d, order=order).tobytes() == x.tobytes()
        for c in rc.CLASSES:
            vol = rc.label_volume(d, c)
            assert np.array_equal(resample_labels(vol, d, c, order=order), np.where((vol >= 0) & (vol < c), vol, 0))
    x[1, 2, 3] = -0.0                         # the sums start at +0.0: order 1 returns the value, not the sign of a zero
    assert resample_image(x, d)[1, 2, 3].tobytes() == np.float32(0.0).tobytes()
    assert resample_image(x, d, order=0).tobytes() == x.tobytes()
    x[1, 1, 1] = np.inf                       # a corner of weight 0 is still multiplied: voxel (1, 1, 1) is corner 111 of (0, 0, 0)
    with np.errstate(invalid='ignore'):
        y = resample_image(x, d)
    assert np.isnan(y[0, 0, 0]) and y[1, 1, 1] == np.inf and np.isfinite(y[2, 2, 2])
    assert resample_image(x, d, order=0).tobytes() == x.tobytes()


def test_resampled_shape():
    shape, real = resampled_shape((256, 256, 33), (1.37, 1.37, 7.7), (1.0, 1.0, 7.7))
    assert shape == (351, 351, 33) and real == (1.37 * 256 / 351, 1.37 * 256 / 351, 7.7 * 33 / 33)
    assert resampled_shape((5, 7, 3), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0))[0] == (3, 4, 2)       # 2.5 -> 3, 3.5 -> 4, 1.5 -> 2
    assert resampled_shape((5, 5, 5), (1.0, 1.0, 1.0), (2.2, 100.0, 0.5))[0] == (2, 1, 10)    # 2.27 -> 2, the floor of 1
    assert resampled_shape((4, 4, 1), (2.0, 1.0, 5.0), (1.0, 1.0, 5.0)) == ((8, 4, 1), (1.0, 1.0, 5.0))
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, float('nan'), 1.0), None):
        with pytest.raises(ValueError):
            resampled_shape((4, 4, 4), bad, (1.0, 1.0, 1.0))
        with pytest.raises(ValueError):
            resampled_shape((4, 4, 4), (1.0, 1.0, 1.0), bad)
    for bad in ((4, 4), (4, 4, 0), (4.0, 4, 4)):
        with pytest.raises(ValueError):
            resampled_shape(bad, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))


@GEO
def test_two_classes_on_a_binary_volume_equal_none(index):
    d, e = rc.GEOMETRIES[index]
    vol = (rc.label_volume(d, 3) == 1).astype(np.uint8)
    for order in (0, 1):
        assert np.array_equal(resample_labels(vol, e, 2, order=order), resample_labels(vol, e, None, order=order))


@GEO
def test_probs_are_the_image_sums_and_their_first_maximum(index):
    d, e = rc.GEOMETRIES[index]
    p = rc.probabilities(d, 5)
    p[:, 3] = p[:, 1]                         # two equal classes everywhere: the lower index
    labels, out = resample_probs(p, e, probs_out=True)
    assert labels.dtype == np.int64 and labels.shape == e and out.dtype == np.float32 and out.shape == (e[0], 5) + e[1:]
    for c in range(5):
        assert out[:, c].tobytes() == resample_image(np.ascontiguousarray(p[:, c]), e).tobytes()
    assert np.array_equal(resample_probs(p, e), labels) and not (labels == 3).any() and (labels == 1).any()
    acc = np.stack([rc.zoom(p[:, c].astype(np.float64), e) for c in range(5)])
    ranked = np.sort(np.delete(acc, 3, axis=0), axis=0)
    decided = ranked[-1] - ranked[-2] > rc.MARGIN
    assert np.array_equal(labels[decided], np.where(acc.argmax(0) == 3, 1, acc.argmax(0))[decided])


def test_argument_errors():
    vol, x = np.zeros((3, 4, 5), np.int64), np.zeros((3, 4, 5), np.float32)
    for bad in (1, 9, 2.0, True, 'per_class'):
        with pytest.raises(ValueError):
            resample_labels(vol, (3, 4, 5), bad)
    for bad in (2, -1, None, True, 1.0):
        with pytest.raises(ValueError):
            resample_labels(vol, (3, 4, 5), 2, order=bad)
        with pytest.raises(ValueError):
            resample_image(x, (3, 4, 5), order=bad)
    for bad in ((3, 4), (3, 4, -1), (3.0, 4, 5), 7, None):
        with pytest.raises(ValueError):
            resample_labels(vol, bad)
        with pytest.raises(ValueError):
            resample_image(x, bad)
        with pytest.raises(ValueError):
            resample_probs(np.zeros((3, 2, 4, 5), np.float32), bad)
    with pytest.raises(ValueError):
        resample_labels(np.zeros((0, 4, 5), np.int64), (3, 4, 5))              # an empty input cannot fill a volume
    with pytest.raises(ValueError):
        resample_labels(vol, (2 ** 20, 2 ** 11, 1))                             # 2^31 voxels
    with pytest.raises(RuntimeError):
        resample_labels(np.zeros((4, 5), np.int64), (3, 4, 5))
    with pytest.raises(RuntimeError):
        resample_labels(x, (3, 4, 5))
    with pytest.raises(RuntimeError):
        resample_image(vol, (3, 4, 5))
    with pytest.raises(RuntimeError):
        resample_image(x[0], (3, 4, 5))
    with pytest.raises(RuntimeError):
        resample_probs(x, (3, 4, 5))
    with pytest.raises(RuntimeError):
        resample_probs(np.zeros((3, 9, 4, 5), np.float32), (3, 4, 5))
    with pytest.raises(RuntimeError):
        resample_probs(np.zeros((3, 2, 4, 5), np.float64), (3, 4, 5))
    assert resample_labels(vol, (0, 4, 5)).shape == (0, 4, 5) and resample_image(x, (3, 0, 5)).shape == (3, 0, 5)


def test_names_are_exported_next_to_the_morphology_names():
    from aide_amd import inference, resample
    for name in ('axis_table', 'resampled_shape', 'resample_image', 'resample_labels', 'resample_probs'):
        assert getattr(inference, name) is getattr(resample, name)
