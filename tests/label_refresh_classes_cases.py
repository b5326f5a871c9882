"""Shared inputs of the per-class label refresh tests (test_label_refresh_classes_host.py, test_gpu_label_refresh_classes.py):
ragged label maps with values >= C and off-palette bank bytes, a plain-loop statement of the counts, hand-sized counts with
ties and NaN scores for the rule, and exact comparisons."""
import numpy as np

# class c <-> bank byte PALETTES[C][c]; the C = 5 and C = 8 tables are not monotone
PALETTES = {2: (0, 63), 3: (0, 63, 126), 5: (0, 252, 63, 126, 189), 8: (7, 0, 63, 126, 189, 252, 1, 200)}
RAGGED = [4, 1, 0, 7, 3, 2, 5]                 # K = 7 with an empty case


def starts(ns):
    return np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)


def random_maps(seed, ns, h, w, palette):
    """-> (labels uint8 [S,h,w] with values 0 .. C + 1 and 255, bank uint8 [S,h,w] of palette bytes and bytes outside it,
    slice_start).  One case predicts nothing, one has an empty pseudo-label."""
    rng = np.random.RandomState(seed)
    c = len(palette)
    st = starts(ns)
    s = int(st[-1])
    lab = rng.randint(0, c + 2, (s, h, w)).astype(np.uint8)
    lab[rng.rand(s, h, w) < 0.03] = 255
    off = [v for v in range(256) if v not in palette]
    pool = np.asarray(list(palette) * 6 + [off[0], off[len(off) // 2], off[-1]], np.uint8)
    bank = pool[rng.randint(0, len(pool), (s, h, w))]
    k = len(ns)
    if k >= 5:
        lab[st[k - 2]:st[k - 1]] = 0
        bank[st[k - 3]:st[k - 2]] = palette[0]
    return lab, bank, st


def long_case_maps(seed, ns, h, w, palette):
    """one case of `ns` slices filled almost entirely with the last class on both sides (2 % of other values, values >= C and
    off-palette bytes among them): a thread of the counts kernel meets the same class at every voxel, so the counter of that
    class is the one that reaches the limit of its packed byte between two flushes"""
    rng = np.random.RandomState(seed)
    c = len(palette)
    lab = np.full((ns, h, w), c - 1, np.uint8)
    bank = np.full((ns, h, w), palette[c - 1], np.uint8)
    other = rng.rand(ns, h, w) < 0.02
    lab[other] = rng.randint(0, c + 2, int(other.sum()))
    other = rng.rand(ns, h, w) < 0.02
    bank[other] = rng.randint(0, 256, int(other.sum()))
    return lab, bank, starts([ns])


def loop_counts(lab, bank, st, palette):
    """the definition as a plain loop over cases and classes"""
    c = len(palette)
    out = np.zeros((len(st) - 1, c, 3), np.int64)
    for k in range(len(st) - 1):
        f, b = lab[st[k]:st[k + 1]], bank[st[k]:st[k + 1]]
        for j in range(c):
            out[k, j] = int(((f == j) & (b == palette[j])).sum()), int((f == j).sum()), int((b == palette[j]).sum())
    return out


def rule_counts(seed, k, c):
    """counts [k,c,3] of small integers: many equal scores (ties across any selection boundary), organs absent on both
    sides, cases without any organ (NaN), and two rows that need the fp64 division; labelled flags for a fifth of the cases"""
    rng = np.random.RandomState(seed)
    p = rng.randint(0, 4, (12, c))
    t = rng.randint(0, 4, (12, c))
    i = (rng.rand(12, c) * (np.minimum(p, t) + 1)).astype(np.int64)
    pool = np.stack([i, p, t], axis=2).astype(np.int64)
    counts = pool[rng.randint(0, 12, k)]                   # twelve distinct rows: every score is shared by many cases
    counts[rng.rand(k) < 0.1, 1:] = 0                      # no organ anywhere: NaN
    if k > 2:
        counts[k // 2, 1] = [16777217, 16777217, 50331653]
        counts[k // 2 + 1, 1:] = 0
        counts[k // 2 + 1, c - 1] = [3, 7, 14]
    return counts, (rng.rand(k) < 0.2).astype(np.uint8)


def same_bits(a, b):
    """float arrays equal in their bit patterns, NaN included; integer arrays equal"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def class_maps(cs, num_classes, seed):
    """two label maps [S,H,W] int64 for the cases of `chaos_cases_multiorgan`: the truth's class indices, shifted, with
    speckle of every class (what the per-class filter removes) and one organ dropped from some cases"""
    from aide_amd.labelbank import CHAOS_PALETTE
    rng = np.random.RandomState(seed)
    truth = cs['truth'].numpy()
    idx = np.zeros(truth.shape, np.int64)
    for c in range(num_classes):
        idx[truth == CHAOS_PALETTE[c]] = c
    out = []
    st = cs['slice_start']
    for n in range(2):
        m = np.roll(idx, (n + 1, -n), (1, 2))
        noise = rng.rand(*m.shape) < 0.02
        m = np.where(noise, rng.randint(0, num_classes, m.shape), m)
        for k in range(len(st) - 1):
            if rng.rand() < 0.3:
                part = m[st[k]:st[k + 1]]
                part[part == rng.randint(1, num_classes)] = 0
        out.append(m)
    return out
