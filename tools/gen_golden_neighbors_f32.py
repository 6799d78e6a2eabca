#!/usr/bin/env python3
"""Generate tests/golden/neighbors_f32_*.npz by running the REFERENCE's own decoder comparison (container-only).

Models come from the portable PRNG recipes of tests/dictionary_util.py, built with the reference classes
(tools/ref_loader.py); scripts/analysis/analyze_sae.py is loaded by file path as tools/gen_golden_dictionary.py does.
Per case only data is written: the recipe and torch.topk(decoder_cosine_similarity(lhs, rhs), k + 1) -- values and
indices, k = 10 -- which is the reference's route to the k nearest atoms of an fp32 dictionary.

The tests compare values at 1e-5 and indices only in rows whose recorded consecutive gaps all exceed 2e-5
(tests/neighbors_f32_util.py); this tool asserts that at least 90 % of every case's rows are such rows.

Run:  python tools/gen_golden_neighbors_f32.py        (needs the reference checkout; CPU only, seconds)
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

import neighbors_f32_util as U  # noqa: E402
from gen_golden_dictionary import load_analyze_sae, wrapper  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"


def main():
    ref = load_reference()
    an = load_analyze_sae(ref)
    OUT.mkdir(parents=True, exist_ok=True)
    k = U.GOLDEN_K
    for name, case in U.GOLDEN_CASES.items():
        lhs, rhs = U.golden_models(ref, case)
        a, b = U.golden_atoms(case)
        with torch.no_grad():
            m = an.decoder_cosine_similarity(wrapper(ref, lhs), wrapper(ref, lhs if rhs is None else rhs))
            top = torch.topk(m, k + 1, dim=1)
        values, indices = top.values.numpy().astype(np.float32), top.indices.numpy().astype(np.int64)
        assert m.shape == (a.shape[0], (a if b is None else b).shape[0]), "the numpy restatement of the recipe disagrees"
        c64, _ = U.cosines_f64(a, b)
        dev = float(np.abs(values.astype(np.float64) - np.take_along_axis(c64, indices, 1)).max())
        assert dev <= U.VALUE_ATOL, f"{name}: the reference is {dev:.3g} from fp64 on the restated atoms"
        share = float(U.clear_rows(values).mean())
        assert share >= 0.9, f"{name}: only {share:.1%} of the rows have clear gaps"
        D, H, Hr = U.case_sizes(case)
        meta = {"lhs": case["lhs"], "rhs": case["rhs"], "D": D, "H": H, "rhs_H": Hr, "k": k, "torch": torch.__version__}
        path = OUT / f"{name}.npz"
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), values=values,
                            indices=indices, clear_share=np.float64(share), ref_fp64_maxdev=np.float64(dev))
        print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  matrix {tuple(m.shape)}  clear rows {share:.1%}  "
              f"ref_fp64_maxdev {dev:.3g}")


if __name__ == "__main__":
    main()
