#!/usr/bin/env python3
"""CPU model of the two choices that decide how many 32-point tiles a wave of the in-loop search scans (r21): the node of the
neighbour the query order sorts by (128-, 64- or 32-point k-d node) and the size of a work item (128, 64 or 32 points).
A model, not a measurement of the fit: a floor of 3000 points / m^2 with 5 mm noise (synth.make_scene's floor), k-d median splits
down to 32-point leaves, 64 000 queries 5-30 cm above it, groups of 32 in key order (ties by query index); a group scans every item
whose box lies within sqrt(best) of at least one of its queries.  Prints tiles scanned per group, fresh and with the order 3 cm
stale (keys from the neighbours of the positions 3 cm ago).  numpy only, seeded.   python tools/nn_group_model.py [queries]"""
import sys

import numpy as np

AREA, DENSITY, NQ = 8.0, 3000, int(sys.argv[1]) if len(sys.argv) > 1 else 64000


def kd_order(xyz):
    """positions in k-d order: median splits along the widest axis down to 32-point leaves (power-of-two point count)"""
    order = np.arange(len(xyz))
    size = len(xyz)
    while size > 32:
        for a in range(0, len(xyz), size):
            seg = order[a:a + size]
            p = xyz[seg]
            ax = np.argmax(p.max(0) - p.min(0))
            order[a:a + size] = seg[np.argsort(p[:, ax], kind="stable")]
        size //= 2
    return order


def nearest(q, pts):
    best = np.empty(len(q))
    idx = np.empty(len(q), np.int64)
    for a in range(0, len(q), 2000):
        d = ((q[a:a + 2000, None, :] - pts[None, :, :]) ** 2).sum(-1)
        idx[a:a + 2000] = d.argmin(1)
        best[a:a + 2000] = d[np.arange(d.shape[0]), idx[a:a + 2000]]
    return best, idx


def tiles_per_group(q, best, key, lo, hi, item_points):
    """mean tiles scanned by a group of 32 queries in key order; lo / hi: boxes of the items"""
    perm = np.argsort(key, kind="stable")
    r2 = best[perm]
    qq = q[perm]
    tiles = 0
    groups = 0
    for a in range(0, len(q), 32):
        x = qq[a:a + 32, None, :]
        d = np.maximum(np.maximum(lo[None] - x, x - hi[None]), 0.0)
        reach = ((d ** 2).sum(-1) <= r2[a:a + 32, None]).any(0)
        tiles += reach.sum() * (item_points // 32)
        groups += 1
    return tiles / groups


def main():
    rng = np.random.default_rng(21)
    n = 1 << int(np.floor(np.log2(AREA * DENSITY)))                  # 16 384 points: whole k-d levels
    side = np.sqrt(n / DENSITY)
    xyz = np.concatenate([rng.uniform(0, side, (n, 2)), rng.normal(0, 0.005, (n, 1))], 1)
    pts = xyz[kd_order(xyz)]
    boxes = {}
    for size in (128, 64, 32):
        p = pts.reshape(-1, size, 3)
        boxes[size] = (p.min(1), p.max(1))
    q = np.concatenate([rng.uniform(0.3, side - 0.3, (NQ, 2)), rng.uniform(0.05, 0.30, (NQ, 1))], 1)
    best, pos = nearest(q, pts)
    print(f"{n} floor points on {side:.2f} x {side:.2f} m, {NQ} queries; tiles scanned per group of 32")
    print(f"{'sort key (neighbour node)':28s} {'items of 128':>13s} {'items of 64':>12s} {'items of 32':>12s}")
    for shift, name in ((7, "128-point (before r21)"), (6, "64-point"), (5, "32-point")):
        row = [tiles_per_group(q, best, pos >> shift, *boxes[size], size) for size in (128, 64, 32)]
        print(f"{name:28s} {row[0]:13.1f} {row[1]:12.1f} {row[2]:12.1f}")
    # the order 3 cm stale: the queries moved since the sort, the keys are the old neighbours'
    ang = rng.uniform(0, 2 * np.pi, NQ)
    q2 = q + 0.03 * np.stack([np.cos(ang), np.sin(ang), np.zeros(NQ)], 1)
    best2, _ = nearest(q2, pts)
    print("with the order 3 cm stale:")
    for shift, size, name in ((7, 128, "128-point key, quarter items"), (5, 128, "tile key, quarter items"), (5, 64, "tile key, 64-point items")):
        print(f"{name:34s} {tiles_per_group(q2, best2, pos >> shift, *boxes[size], size):6.1f}")


if __name__ == "__main__":
    main()
