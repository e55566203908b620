#!/usr/bin/env python3
"""Generates tests/golden/ref_chunk_dataset/chunk_dataset.npz -- what the
REFERENCE's chunk datasets return for a fixed random stream, the golden vectors
of chunks.draw_ranges + chunks.range_features_host and of ChunkStore.batch.
Run where a checkout of the reference is at hand; the tests read the committed
output only.

  python tests/golden/ref_chunk_dataset/make_fixtures.py --reference <kf2vec checkout>

How: kf2vec/datasets.py is loaded from the checkout by file path (it imports
torch, pandas and numpy only) and its own classes are run:

  * Dataset_chunks_2rows (datasets.py:7-101) on uint16 DataFrames, as
    my_read_csv_chunk parses them (utils.py:402-405);
  * Dataset_chunks_2rows_numpy (datasets.py:103-199) on uint16 arrays;
  * each again on the same counts capped at 255 as uint8, what
    my_read_csv_chunk_capped gives (utils.py:412-423),

with features_scaler = 1e4 (train_model_set_chunks.py:74).  Every run seeds the
global numpy stream (np.random.seed) and asks for the same sequence of items.

The file holds data only: the count matrices (nbins = 32; genomes of 1, 3, 5, 7
and 40 windows, the second all zeros, the third with one zero row; counts up
to 400 so the cap bites), the seed, the item sequence and each run's float64 Z
and labels y.
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20241
NBINS = 32
WINDOWS = [1, 3, 5, 7, 40]
ITEMS = 240
SCALER = 1e4


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (holds kf2vec/datasets.py)")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_datasets", os.path.join(args.reference, "kf2vec", "datasets.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rs = np.random.RandomState(SEED)
    counts = [rs.randint(0, 401, size=(c, NBINS)).astype(np.uint16) for c in WINDOWS]
    counts[1][:] = 0
    counts[2][3] = 0
    idx = rs.randint(0, len(WINDOWS), size=ITEMS).astype(np.int64)
    idx[: len(WINDOWS)] = np.arange(len(WINDOWS))   # every genome at least once
    names = ["g{}".format(i) for i in range(len(WINDOWS))]
    labels = {n: i for i, n in enumerate(names)}

    out = {"seed": np.int64(SEED), "idx": idx, "scaler": np.float64(SCALER)}
    for g, c in enumerate(counts):
        out["counts_{}".format(g)] = c
    for tag, cap in (("", False), ("_cap", True)):
        data = [np.minimum(c, 255).astype(np.uint8) if cap else c for c in counts]
        runs = {"frame": ref.Dataset_chunks_2rows([pd.DataFrame(d) for d in data], names, labels, SCALER),
                "numpy": ref.Dataset_chunks_2rows_numpy(data, names, labels, SCALER)}
        for kind, ds in runs.items():
            np.random.seed(SEED)
            with np.errstate(invalid="ignore", divide="ignore"):
                items = [ds[int(i)] for i in idx]
            out["Z_{}{}".format(kind, tag)] = np.stack([np.asarray(z, dtype=np.float64) for z, _ in items])
            out["y_{}{}".format(kind, tag)] = np.asarray([y for _, y in items], dtype=np.int64)
    path = os.path.join(HERE, "chunk_dataset.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
