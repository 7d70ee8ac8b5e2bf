"""Generates tests/golden/paper_oracle.npz: the points and the oracle co-clustering matrices of the three N = 100, K = 10
paper datasets, as the Julia package stored them in its data/example_datasets.h5 (provenance: src/example_data.jl:40-71 of
the reference; parameters α = 10, radius = 1, σ = 0.25 / 0.2 / 0.18, dim = 10 / 50 / 10).  DATA only.

  python tests/golden/make_paper_oracle.py PATH/TO/example_datasets.h5

The blocks are contiguous little-endian f64 in that file (HDF5 superblock v0), read at the byte offsets below.  Each is
checked before it is written: the points reproduce the distance matrices of paper_datasets.npz to < 1e-9, and every
oracle matrix is exactly symmetric with entries in [0, 1]."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = {1: (4096, 10), 2: (175024, 50), 3: (377952, 10)}   # (offset, dim), 100 points, point-major
ORACLE = {1: 92976, 2: 295904, 3: 470048}                    # 100 × 100


def extract(path):
    b = open(path, "rb").read()
    ref = np.load(os.path.join(HERE, "paper_datasets.npz"))
    out = {}
    for d, (off, dim) in POINTS.items():
        X = np.frombuffer(b, dtype="<f8", count=100 * dim, offset=off).reshape(100, dim).copy()
        D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
        assert np.abs(D - ref[f"D{d}"]).max() < 1e-9, d
        O = np.frombuffer(b, dtype="<f8", count=100 * 100, offset=ORACLE[d]).reshape(100, 100).copy()
        assert np.array_equal(O, O.T) and O.min() >= 0 and O.max() <= 1, d
        out[f"points{d}"] = X
        out[f"oracle{d}"] = O
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "paper_oracle.npz"), **extract(sys.argv[1]))
