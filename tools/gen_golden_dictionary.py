#!/usr/bin/env python3
"""Generate tests/golden/dictionary_*.npz by running the REFERENCE's own decoder comparison (container-only).

Models come from the portable PRNG recipes of tests/dictionary_util.py (quantizedsae_amd/synthetic.py), built with the
reference classes (tools/ref_loader.py).  scripts/analysis/analyze_sae.py is loaded by file path with
`quantized_sae.inference.framework` pre-registered as the framework module ref_loader already loads -- the reference
package itself is never imported (its __init__ starts a training run).  Only data is written: the recipe, row and
column max / argmax, the mean, the mean of the top 100 row maxima and 16 strided rows of the matrix.

Run:  python tools/gen_golden_dictionary.py        (needs the reference checkout; CPU only, seconds)
"""
from __future__ import annotations

import importlib.util
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

import dictionary_util as U  # noqa: E402
from ref_loader import REF_ROOT, load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
D, H = 64, 512

CASES = {
    "dictionary_binary": dict(lhs={"variant": "binary", "seed": 41}, rhs={"variant": "baseline", "seed": 42}),
    "dictionary_matryoshka": dict(lhs={"variant": "matryoshka", "seed": 43}, rhs={"variant": "baseline", "seed": 42}),
    "dictionary_residual": dict(lhs={"variant": "residual", "seed": 44}, rhs={"variant": "baseline", "seed": 42}),
    "dictionary_self": dict(lhs={"variant": "baseline", "seed": 42}, rhs={"variant": "baseline", "seed": 42}),
    "dictionary_zero_atom": dict(lhs={"variant": "baseline", "seed": 45, "zero_atom": 7},
                                 rhs={"variant": "baseline", "seed": 42}),
    "dictionary_square": dict(lhs={"variant": "binary", "seed": 46}, rhs={"variant": "baseline", "seed": 47}, D=64, H=64),
}


def load_analyze_sae(ref):
    for name in ("quantized_sae", "quantized_sae.inference"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    sys.modules["quantized_sae.inference.framework"] = ref.framework
    path = REF_ROOT / "scripts" / "analysis" / "analyze_sae.py"
    spec = importlib.util.spec_from_file_location("ref_analyze_sae", str(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wrapper(ref, model):
    fw = ref.framework
    getter = {"BinarySAE": fw._decoder_binary, "QuantizedMatryoshkaSAE": fw._decoder_quantized,
              "ResidualQuantizedSAE": fw._decoder_residual}.get(type(model).__name__, fw._decoder_baseline)
    entry = fw.SAERegistryEntry(name=type(model).__name__, constructor=type(model), checkpoint_path=Path("."),
                                checkpoint_format="torch", kwargs={}, forward_adapter=None, decoder_getter=getter)
    return fw.SAEWrapper(entry, model, "cpu")


def main():
    ref = load_reference()
    an = load_analyze_sae(ref)
    OUT.mkdir(parents=True, exist_ok=True)
    for name, case in CASES.items():
        d, h = case.get("D", D), case.get("H", H)
        lhs = wrapper(ref, U.build(ref, case["lhs"], d, h))
        rhs = wrapper(ref, U.build(ref, case["rhs"], d, h))
        with torch.no_grad():
            m = an.decoder_cosine_similarity(lhs, rhs).numpy()
        k = min(100, m.shape[1])
        meta = {"D": d, "H": h, "lhs": case["lhs"], "rhs": case["rhs"], "self": case["lhs"] == case["rhs"],
                "n_bits": U.N_BITS, "rows_stride": max(1, m.shape[0] // 16)}
        rows = np.arange(0, m.shape[0], meta["rows_stride"])[:16]
        arrays = dict(row_max=m.max(1), row_argmax=m.argmax(1).astype(np.int64), col_max=m.max(0),
                      col_argmax=m.argmax(0).astype(np.int64), mean=np.float64(m.mean()),
                      mean_top=np.float64(torch.topk(torch.from_numpy(m.max(1)), k).values.mean().item()),
                      rows=rows.astype(np.int64), matrix_rows=m[rows])
        path = OUT / f"{name}.npz"
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
        print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  atoms {m.shape}")


if __name__ == "__main__":
    main()
