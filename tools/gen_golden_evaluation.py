#!/usr/bin/env python3
"""Generate tests/golden/evaluation_*.npz by running the REFERENCE's own evaluation scripts (container-only).

scripts/evaluation/estimate_quantization_error.py is loaded by file path after tools/ref_loader.py has registered the
reference's model classes under the legacy module names it imports; its recover_float_decoder, recover_quantized_decoder,
summarize_error, summarize_matrix and find_max_diff_entry run on reference BinarySAE checkpoints at H = 64, D = 32,
n_bits in {2, 4, 8}: kaiming-initialised (unpolarised) and polarised (logits +-8).  scripts/evaluation/
estimate_baseline_error.py is loaded the same way, with a stub `hidden_state_dataset` module whose dataset class serves a
saved tensor, and its function runs in a temporary working directory holding one 2100-row chunk with a NaN row inside the
second 1024-row batch.

Only data is written: the logits, the rows, and the numbers the reference's functions returned.

Run:  python tools/gen_golden_evaluation.py        (needs the reference checkout; CPU only, seconds)
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from ref_loader import REF_ROOT, load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
H, D, GAMMA = 64, 32, 4.0
ROWS, DATA_D, NAN_ROW = 2100, 16, 1500


def _load_script(name: str):
    spec = importlib.util.spec_from_file_location(f"ref_{name}", str(REF_ROOT / "scripts" / "evaluation" / f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quantization():
    load_reference()
    q = _load_script("estimate_quantization_error")
    arrays, meta = {}, {"H": H, "D": D, "gamma": GAMMA, "torch": torch.__version__, "cases": []}
    for n in (2, 4, 8):
        for kind in ("kaiming", "polarised"):
            torch.manual_seed(100 + n)
            model = q.BinarySAE(D, H, gamma=GAMMA, n_bits=n).eval()
            if kind == "polarised":
                with torch.no_grad():
                    model.decoder.weight.copy_(torch.where(model.decoder.weight > 0, 8.0, -8.0))
            w_float, w_quant = q.recover_float_decoder(model), q.recover_quantized_decoder(model)
            stats = q.summarize_error(w_quant - w_float)
            stats.update(q.summarize_matrix(w_float, "float"))
            stats.update(q.summarize_matrix(w_quant, "quant"))
            entry = dict(q.find_max_diff_entry(model, w_float, w_quant))
            bits = entry.pop("bit_details")
            name = f"{kind}_n{n}"
            arrays[f"{name}_logits"] = model.decoder.weight.detach().numpy().copy()
            arrays[f"{name}_bit_details"] = np.array([[b[k] for k in ("bit_index", "logit", "prob", "hard", "bit_weight",
                                                                        "float_contrib", "quant_contrib")] for b in bits], np.float64)
            meta["cases"].append({"name": name, "n_bits": n, "step": model.decoder.quantization_step, "stats": stats, "entry": entry,
                                  "report": q.format_report(stats, {**entry, "bit_details": bits})})
    path = OUT / "evaluation_quantization.npz"
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  {len(meta['cases'])} checkpoints")


def baseline():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(ROWS, DATA_D, generator=g) * 2.5 + 0.3
    x[NAN_ROW, 5] = float("nan")
    stub = types.ModuleType("hidden_state_dataset")

    class HiddenStatesTorchDataset(torch.utils.data.Dataset):
        def __init__(self, path):
            self.rows = torch.load(path)

        def __len__(self):
            return self.rows.shape[0]

        def __getitem__(self, i):
            return self.rows[i]

    stub.HiddenStatesTorchDataset = HiddenStatesTorchDataset
    sys.modules["hidden_state_dataset"] = stub
    b = _load_script("estimate_baseline_error")
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "dataset"))
        torch.save(x, os.path.join(tmp, "dataset", "the_pile_hidden_states_L3_0.pt"))
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                result = b.estimate_baseline_error(num_files=1)
        finally:
            os.chdir(cwd)
    meta = {"rows": ROWS, "D": DATA_D, "nan_row": NAN_ROW, "batch_rows": 1024, "torch": torch.__version__,
            "result": {k: (int(v) if k == "total_samples" else float(v)) for k, v in result.items()}}
    path = OUT / "evaluation_baseline.npz"
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), x=x.numpy())
    print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  {meta['result']}")


if __name__ == "__main__":
    quantization()
    baseline()
