#!/usr/bin/env python3
"""Writes tests/golden/cloud_nn_golden_v1.npz: two clouds of about 3000 fp32 points on a wavy surface and, per query point,
the float64 distance to its nearest target point, found with scipy.spatial.cKDTree on the fp32 coordinates widened to
float64.  Uses numpy and scipy only, nothing from this repository: an independent statement of "nearest neighbour" for
tests/test_cloud_gpu.py.  The seed is chosen so that no query's distance lies within a relative 1e-5 of one of the radii the
test uses (checked below), so the test has a verdict for every query."""
import os

import numpy as np
from scipy.spatial import cKDTree

RADII = np.array([0.03, 0.12])
SEED = 20240


def surface(rng, n, noise):
    u = rng.uniform(-2.0, 2.0, n)
    v = rng.uniform(-1.5, 1.5, n)
    w = 0.4 * np.sin(2.1 * u) * np.cos(1.7 * v) + 0.1 * u
    p = np.stack([u + 7.0, v - 3.0, w + 12.0], 1) + rng.normal(0.0, noise, (n, 3))
    return p.astype(np.float32)


def main():
    rng = np.random.default_rng(SEED)
    targets = surface(rng, 3000, 0.0)
    queries = np.concatenate([surface(rng, 2800, 0.02), (rng.uniform(-3, 3, (200, 3)) + [7.0, -3.0, 12.0]).astype(np.float32)])
    dist, _ = cKDTree(targets.astype(np.float64)).query(queries.astype(np.float64), k=1)
    for r in RADII:
        band = (dist >= r * (1 - 1e-5)) & (dist <= r * (1 + 1e-5))
        assert not band.any(), f"seed {SEED}: {int(band.sum())} queries within 1e-5 of radius {r}; choose another seed"
        print(f"radius {r}: {int((dist < r).sum())} of {len(dist)} queries have a neighbour")
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cloud_nn_golden_v1.npz")
    np.savez_compressed(out, targets=targets, queries=queries, distance=dist.astype(np.float64), radii=RADII)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
