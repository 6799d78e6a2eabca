#!/usr/bin/env python3
"""Generate tests/golden/kmeans_inspector_ternary.npz by running the REFERENCE's own ``k_means_analysis`` (container-only).

src/quantized_sae/utils/inspector.py is loaded by file path exactly as tools/gen_golden_dictionary_neighbors.py loads it
(stand-in modules for what cannot be imported, the failure of the module-level lines caught, an instance made with
object.__new__).  ``kmeans_pytorch`` is not installed, so the name ``kmeans`` in the reference module is a stub that
returns labels and centers supplied here: one Lloyd run of the numpy restatement (tests/kmeans_util.py) on a small
ternary dictionary of uneven sparsity, N = 300, D = 64, C = 7, one cluster forced empty.  What is recorded is what the
reference's OWN code computes around that call: ``cluster_ids_by_group`` and ``center_features`` (cosine only: the
euclidean branch of the reference raises AttributeError through a misspelt attribute).

Only data is written: the recipe, the supplied labels and centers, the groups (ragged, as offsets + members) and the
center features.

Run:  python tools/gen_golden_kmeans.py        (needs the reference checkout; CPU only, seconds)
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import kmeans_util as U  # noqa: E402
from gen_golden_dictionary_neighbors import load_inspector_class  # noqa: E402


def main():
    Inspector = load_inspector_class()
    a = U.golden_atoms()
    labels, centers = U.golden_lloyd(a)
    assert centers.shape == (U.GOLDEN_C, U.GOLDEN_D) and not (labels == U.GOLDEN_EMPTY).any() and (labels >= 0).all()
    calls = []

    def kmeans_stub(X, num_clusters, distance, device):
        calls.append((tuple(X.shape), num_clusters, distance, str(device)))
        return torch.from_numpy(labels.astype(np.int64)), torch.from_numpy(centers.copy())

    Inspector.k_means_analysis.__globals__["kmeans"] = kmeans_stub
    ins = object.__new__(Inspector)
    ins.dictionary_in_ternary = torch.from_numpy(a.copy())
    ids, cc, groups, center_features = ins.k_means_analysis(U.GOLDEN_C, "cosine")
    assert calls == [((U.GOLDEN_N, U.GOLDEN_D), U.GOLDEN_C, "cosine", "cpu")]
    center_features = [int(f) for f in center_features]
    # the restatement evaluates the same expression in fp64; a near-tie that fp32 resolves differently would show here
    assert [list(map(int, g)) for g in groups] == U.groups(labels, U.GOLDEN_C)
    assert center_features == U.center_features(a, labels, centers, "cosine"), "fp32 and fp64 disagree: pick another seed"
    assert center_features[U.GOLDEN_EMPTY] == -1 and groups[U.GOLDEN_EMPTY] == []
    sizes = [len(g) for g in groups]
    meta = {"N": U.GOLDEN_N, "D": U.GOLDEN_D, "C": U.GOLDEN_C, "seed": U.GOLDEN_SEED, "empty": U.GOLDEN_EMPTY,
            "type": "cosine", "torch": torch.__version__}
    path = U.GOLDEN / f"{U.GOLDEN_NAME}.npz"
    np.savez_compressed(
        path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), atoms=a.astype(np.int8),
        labels=labels.astype(np.int64), centers=centers.astype(np.float32),
        group_offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
        group_members=np.array([m for g in groups for m in g], dtype=np.int64),
        center_features=np.array(center_features, dtype=np.int64))
    print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  sizes {sizes}  center features {center_features}")


if __name__ == "__main__":
    main()
