"""Shared by test_lcc_classes_host.py and test_gpu_lcc_classes.py: small label volumes for the per-class largest-component
filter (aide_amd.inference.keep_largest_per_class), chosen where the kernels can go wrong, and an independent statement of
the definition.  The device tile is 4 x 16 x 16 over the logical (i0, i1, i2): shapes are odd, below one tile, exactly one
tile and several tiles; blobs cross tile borders; ties sit inside one tile and across tiles.

cases()      -> [(name, volume, num_classes)]: int64 numpy volumes, one of them a non-contiguous view
flood_fill() -> (uint8 volume, int64 stats [C, 3]) by breadth-first search over face neighbours, per class"""
from collections import deque

import numpy as np

RANDOM_SHAPES = ((5, 17, 33), (4, 16, 16), (1, 1, 1), (9, 40, 21), (3, 1, 50))


def flood_fill(vol, c):
    """Per class 1 .. c - 1: components by BFS over the six face neighbours, the one with the most voxels kept, ties to the
    component whose first voxel has the lowest raster index of the logical volume.  No library call but numpy's zeros."""
    vol = np.asarray(vol)
    d0, d1, d2 = vol.shape
    val = vol.tolist()                            # nested lists in logical order, whatever the strides
    seen = np.zeros(vol.shape, bool)
    out = np.zeros(vol.shape, np.uint8)
    stats = np.zeros((c, 3), np.int64)
    best = {}                                     # class -> (area, -first raster index, voxels)
    for z in range(d0):
        for y in range(d1):
            for x in range(d2):
                v = val[z][y][x]
                if seen[z, y, x] or not 1 <= v < c:
                    continue
                seen[z, y, x] = True
                todo, blob = deque([(z, y, x)]), []
                while todo:
                    a, b, e = todo.popleft()
                    blob.append((a, b, e))
                    for p, q, r in ((a - 1, b, e), (a + 1, b, e), (a, b - 1, e), (a, b + 1, e), (a, b, e - 1), (a, b, e + 1)):
                        if 0 <= p < d0 and 0 <= q < d1 and 0 <= r < d2 and not seen[p, q, r] and val[p][q][r] == v:
                            seen[p, q, r] = True
                            todo.append((p, q, r))
                stats[v, 0] += 1
                stats[v, 1] += len(blob)
                cand = (len(blob), -((z * d1 + y) * d2 + x))
                if v not in best or cand > best[v][:2]:
                    best[v] = cand + (blob,)
    for v, (area, _, blob) in best.items():
        stats[v, 2] = area
        for a, b, e in blob:
            out[a, b, e] = v
    return out, stats


def serpentine(d0, d1, d2, value):
    """One component that winds through the whole volume: every other row of every other plane, rows joined at alternating
    ends, planes joined at one corner."""
    v = np.zeros((d0, d1, d2), np.int64)
    for z in range(0, d0, 2):
        for y in range(0, d1, 2):
            v[z, y, :] = value
            if y + 1 < d1:
                v[z, y + 1, d2 - 1 if (y // 2) % 2 == 0 else 0] = value
        if z + 1 < d0:
            v[z + 1, d1 - 1 if d1 % 2 == 1 else d1 - 2, 0] = value
    return v


def serpentine_case():
    """class 2 winds through every tile of (9, 33, 35); compact class-1 and class-3 blobs with fewer voxels in the planes it
    leaves free, face-adjacent to it"""
    v = serpentine(9, 33, 35, 2)
    v[1, 2:6, 5:9] = 1                            # 16 voxels, the class-1 winner
    v[3, 20:23, 14:18] = 1                        # 12, across the tile border at i2 = 16
    v[5, 10:13, 10:14] = 3                        # 12, the class-3 winner
    v[7, 15:17, 30:34] = 3                        # 8, across the borders at i1 = 16 and i2 = 32
    return v


def ties_case():
    """(9, 20, 40), C = 5.  Class 1: two blobs of 12 voxels in different tiles, A first in (i0, i1, i2) order, B first in
    (i2, i0, i1) order.  Class 3: two blobs of 3 voxels inside one tile.  Class 2: one blob of 12 voxels, the area of the
    class-1 winner, across the tile borders at i0 = 4 and i2 = 32.  Class 4: single voxels only (every one a tie)."""
    v = np.zeros((9, 20, 40), np.int64)
    v[0:2, 0:2, 20:23] = 1                        # A
    v[5:7, 17:19, 0:3] = 1                        # B
    v[0, 4, 17:20] = 3
    v[2, 8, 20:23] = 3
    v[3:5, 5:7, 30:33] = 2
    v[8, 0, 39] = 4
    v[8, 19, 0] = 4
    v[0, 19, 39] = 4
    return v


def adjacent_case():
    """two classes that meet at a tile border (i2 = 16) and a third that touches both inside the tiles: no merge"""
    v = np.zeros((5, 20, 40), np.int64)
    v[:, :, :16] = 1
    v[:, :, 16:] = 2
    v[1:4, 3:9, 10:22] = 3
    v[4, 19, 10] = 2                              # a class-2 voxel enclosed by class 1 and the walls: its own blob
    return v


def cases():
    out = []
    for n, shape in enumerate(RANDOM_SHAPES):
        for density in (0.3, 0.7):
            rng = np.random.RandomState(100 * n + int(density * 10))
            v = np.where(rng.rand(*shape) < density, rng.randint(1, 5, shape), 0).astype(np.int64)
            out.append(('random %s %.1f' % ('x'.join(map(str, shape)), density), v, 5))
    rng = np.random.RandomState(7)
    out.append(('blocks', np.kron(rng.randint(0, 5, (3, 10, 7)), np.ones((3, 4, 3), np.int64)).astype(np.int64), 5))
    out.append(('serpentine', serpentine_case(), 5))
    t = ties_case()
    out.append(('ties', t, 5))
    out.append(('ties permuted', t.transpose(2, 0, 1), 5))              # a view: logical (40, 9, 20), strides of (9, 20, 40)
    out.append(('class absent', np.array([0, 1, 3, 4])[rng.randint(0, 4, (5, 17, 33))].astype(np.int64), 5))
    out.append(('all zero', np.zeros((5, 17, 33), np.int64), 5))
    out.append(('out of range', np.array([-3, 0, 1, 2, 3, 4, 5, 7])[rng.randint(0, 8, (9, 40, 21))].astype(np.int64), 5))
    out.append(('adjacent', adjacent_case(), 5))
    for shape, density in (((5, 17, 33), 0.3), ((5, 17, 33), 0.6), ((9, 40, 21), 0.45)):
        out.append(('binary %s %.2f' % ('x'.join(map(str, shape)), density),
                    (rng.rand(*shape) < density).astype(np.int64), 2))
    v8 = rng.randint(0, 8, (9, 40, 21)).astype(np.int64)
    assert set(np.unique(v8).tolist()) == set(range(8))
    out.append(('eight classes', v8, 8))
    return out
