#!/usr/bin/env python3
"""Generate tests/golden/nearest_atoms_*.npz by running the REFERENCE's own inspector class (container-only).

src/quantized_sae/utils/inspector.py is loaded by file path with stub modules for what it imports and this machine
lacks: `ternary_SAE` is the reference's ternary module as tools/ref_loader.py loads it; `detokenizer`,
`anthropic_handler` and `kmeans_pytorch` are empty stand-ins (nothing recorded here calls them).  The file's
module-level lines build an inspector and call it; with no checkpoint on disk that call fails, after the class object
is in the module namespace.  The failure is caught, an instance is made with object.__new__ and its
`dictionary_in_ternary` is set from a reference model built from a portable recipe (tests/dictionary_neighbors_util.py).
The reference has no inspector for BinarySAE: the binary fixture feeds the reference BinarySAE's
quantized_int_weights() through the same reference methods.

Only data is written: the recipe, the atoms, per row the k + 1 smallest distances of the reference's matrix and their
indices (k = 10), the scalar results, and ref_fp64_maxdev -- the largest deviation of the reference's fp32 distance
matrix from an fp64 evaluation of the same atoms, which sets the tests' tolerance.

Run:  python tools/gen_golden_dictionary_neighbors.py        (needs the reference checkout; CPU only, seconds)
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import dictionary_neighbors_util as U  # noqa: E402
from ref_loader import REF_ROOT, load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
PAIRS = [(0, 1), (5, 400), (7, 300), (9, 130), (17, 511), (0, 0)]      # distance(f1, f2) probes
SAME = [[5, 400], [9, 130, 511], [1, 2, 3]]                             # check_same_entries probes


def load_inspector_class():
    load_reference()                                         # registers the reference's ternary module as ref_ternary
    sys.modules["ternary_SAE"] = sys.modules["ref_ternary"]
    for name in ("detokenizer", "anthropic_handler"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["anthropic_handler"].AnthropicHandler = lambda *a, **k: None
    km = types.ModuleType("kmeans_pytorch")
    km.kmeans = None
    sys.modules.setdefault("kmeans_pytorch", km)
    path = REF_ROOT / "src" / "quantized_sae" / "utils" / "inspector.py"
    spec = importlib.util.spec_from_file_location("ref_inspector", str(path))
    mod = importlib.util.module_from_spec(spec)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            spec.loader.exec_module(mod)
    except Exception as e:                                   # the module-level call on an inspector without a checkpoint
        print(f"  (reference module-level code stopped as expected: {type(e).__name__}: {e})")
    return mod.TernarySparseAutoencoderInspector


def reference_atoms(ref, spec):
    model = U.golden_model(ref, spec)
    with torch.no_grad():
        if spec["variant"] == "binary":
            return model.decoder.quantized_int_weights().detach().float().contiguous()
        w, thr = model.decoder.weight, model.decoder.threshold   # inspector.py:32-39
        hard = torch.sign(w) * (torch.abs(w) >= thr).float()
        return hard.permute(1, 0).contiguous().detach()


def main():
    ref = load_reference()
    Inspector = load_inspector_class()
    OUT.mkdir(parents=True, exist_ok=True)
    k = U.GOLDEN_K
    for name, spec in U.GOLDEN_CASES.items():
        ins = object.__new__(Inspector)
        ins.dictionary_in_ternary = reference_atoms(ref, spec)
        atoms = ins.dictionary_in_ternary.numpy()
        assert np.array_equal(atoms, np.round(atoms)) and np.abs(atoms).max() <= 128
        a8 = atoms.astype(np.int8)
        assert np.array_equal(a8, U.golden_atoms(spec)), "the numpy restatement of the recipe disagrees with the reference"
        dist, knn_idx = ins.calculate_k_nearest_features_cluster(k + 1, "cosine")
        order = np.argsort(dist, axis=1, kind="stable")[:, :k + 1]
        nn_dist = np.take_along_axis(dist, order, 1)
        # sklearn's own neighbour indices agree with the sorted matrix up to the order of equal distances
        assert np.allclose(np.take_along_axis(dist, knn_idx, 1), nn_dist, atol=0, rtol=0)
        dev = float(np.abs(dist.astype(np.float64) - np.maximum(1.0 - U.cosines_f64(a8), 0.0)).max())
        tol = dev + 3e-7
        clear = (nn_dist[:, k].astype(np.float64) - nn_dist[:, k - 1].astype(np.float64)) > 2 * tol
        share = float(clear.mean())
        assert share >= 0.9, f"{name}: only {share:.1%} of the rows have a clear k-th neighbour"
        with contextlib.redirect_stdout(io.StringIO()):
            n_dup = ins.count_duplicates()
        vals, counts = np.unique(a8, return_counts=True)
        same = [ins.check_same_entries(s) for s in SAME]
        meta = {"recipe": spec, "D": U.GOLDEN_D, "H": U.GOLDEN_H, "k": k, "n_bits": U.N_BITS, "gamma": U.GAMMA,
                "pairs": PAIRS, "same": SAME, "torch": torch.__version__}
        arrays = dict(
            atoms=a8, nn_dist=nn_dist.astype(np.float32), nn_index=order.astype(np.int64),
            ref_fp64_maxdev=np.float64(dev), clear_share=np.float64(share),
            zero_entries=np.int64(ins.zero_entries()), count_duplicates=np.int64(n_dup),
            sparsity_rate=np.float64(ins.sparsity_rate()),
            values=vals.astype(np.int64), value_counts=counts.astype(np.int64),
            pair_cosine=np.array([float(ins.distance(a, b, "cosine")) for a, b in PAIRS], dtype=np.float64),
            pair_euclidean=np.array([float(ins.distance(a, b, "euclidean")) for a, b in PAIRS], dtype=np.float64),
            same_count=np.array([c for c, _ in same], dtype=np.int64),
            same_pos=np.concatenate([p[0].numpy() for _, p in same]).astype(np.int64),
        )
        path = OUT / f"{name}.npz"
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
        print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  atoms {a8.shape}  clear rows {share:.1%}  "
              f"ref_fp64_maxdev {dev:.3g}  duplicates {n_dup}  zero atoms {int(arrays['zero_entries'])}")


if __name__ == "__main__":
    main()
