"""Inputs on which the three pseudo-label refresh rules (case bank, per-class bank with C = 2, per-image bank) are defined to
agree, shared by tests/test_refresh_rules_agree_host.py and tests/test_gpu_refresh_shared.py."""
import numpy as np

N = 100                                        # voxels per item


def shared_sums(seed, k, zero_rows=False):
    """-> (sums int64 [k,4] = N / sum p*t / sum p / sum t, labelled uint8 [k], n_select).  Small integers with sum p > 0 in every
    row: many equal scores, a fifth of the rows labelled, and (k > 1) the rows at positions n_select - 1 and n_select of the
    ranking hold the same integers, so one tie crosses the selection boundary.  zero_rows: an eighth of the rows (k >= 8) are
    N / 0 / 0 / 0 instead, the 0 / 0 of the case rules; the tie is placed below them."""
    rng = np.random.RandomState(seed)
    p = rng.randint(1, 7, k)
    t = rng.randint(0, 7, k)
    pt = (rng.randint(0, 7, k) * np.minimum(p, t)) // 6
    sums = np.stack([np.full(k, N), pt, p, t], 1).astype(np.int64)
    if zero_rows:
        sums[rng.permutation(k)[:k // 8], 1:] = 0
    n_select = max(1, k // 4)
    if k > 1:
        with np.errstate(invalid='ignore'):
            d = (2.0 * sums[:, 1] / (sums[:, 2] + sums[:, 3])).astype(np.float32)
        order = np.argsort(d, kind='stable')               # numpy puts NaN last
        sums[order[n_select]] = sums[order[n_select - 1]]
    labelled = (rng.rand(k) < 0.2).astype(np.uint8)
    return sums, labelled, n_select


def counts_c2(sums):
    """the C = 2 counts [k,2,3] = (I, P, T) per class of the same maps: class 1 is the foreground, class 0 its complement"""
    n, pt, p, t = (sums[:, j] for j in range(4))
    return np.stack([np.stack([n - p - t + pt, n - p, n - t], 1), np.stack([pt, p, t], 1)], 1).astype(np.int64)


def boundary_tie(dice, rank, n_select):
    """whether the items ranked n_select - 1 and n_select have the same score"""
    order = np.argsort(rank)
    return dice[order[n_select - 1]] == dice[order[n_select]]


def same_bits(a, b):
    """arrays of one dtype and shape with the same bytes (NaN included)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
