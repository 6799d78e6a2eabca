#!/usr/bin/env python3
"""Generate tests/golden/inspector_overview.npz by running the REFERENCE's own inspector methods (container-only).

The inspector class is loaded as tools/gen_golden_dictionary_neighbors.py loads it (stub modules for what this machine
lacks; the module-level call on an inspector without a checkpoint fails after the class exists).  An instance made with
object.__new__ gets a small reference TernarySparseAutoencoder (D = 16, H = 20, seeded; one unit's encoder bias far below
zero, so that feature never wins) and runs, on 12 lines x 9 tokens:

  linguistic_analyze                    -> feature_activations
  print_feature_activations_overview    -> feature_dict
  check_sensitivity / check_specificity -> both scores for three (feature, targets) pairs, one of whose targets never
                                           appears in a position its feature won

Only data is written: the table, the dict as counts + CSR positions, the token strings, per pair the bool match mask
computed the reference's way (`any(target in token for target in targets)`) and the two scores.

Run:  python tools/gen_golden_inspector_overview.py        (needs the reference checkout; CPU only, seconds)
"""
from __future__ import annotations

import contextlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

from gen_golden_dictionary_neighbors import load_inspector_class  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
LINES, TOKENS, D, H = 12, 9, 16, 20
DEAD = 13                                                       # the feature that never wins
VOCAB = ["it", "It", " it", "me", " Me", "we", "us", " the", "cat", "sat", ".", ",", " I", "item", " of"]


def main():
    ref = load_reference()
    Inspector = load_inspector_class()
    torch.manual_seed(20)
    ins = object.__new__(Inspector)
    ins.sae = ref.TernarySparseAutoencoder(input_dim=D, hidden_dim=H)
    with torch.no_grad():
        ins.sae.encoder[0].bias[DEAD] = -100.0
    g = torch.Generator().manual_seed(21)
    data = torch.randn(LINES, TOKENS, D, generator=g)
    tok_ids = torch.randint(0, len(VOCAB), (LINES, TOKENS), generator=g)
    tokens = [[VOCAB[i] for i in row] for row in tok_ids.tolist()]
    with contextlib.redirect_stdout(io.StringIO()):
        fa = ins.linguistic_analyze(data)
        fd = ins.print_feature_activations_overview(fa)
    fa_np = np.asarray(fa, dtype=np.int64)
    assert fa_np.shape == (LINES, TOKENS) and DEAD not in fd and len(fd) < H
    ranked = sorted(fd, key=lambda f: -fd[f]["cnt"])
    # (feature, targets): two common features with common targets, and one whose target never meets a winning position
    never = None
    for f in ranked:
        for t in VOCAB:
            appears = any(t in tok for row in tokens for tok in row)
            hit = any(t in tokens[line][pos] for line, pos in fd[f]["pos"])
            if appears and not hit:
                never = (f, [t])
                break
        if never:
            break
    assert never is not None
    pairs = [(ranked[0], ["it", "It"]), (ranked[1], ["me", "Me", "we", "us"]), never]
    counts = np.zeros(H, np.int64)
    pos = []
    for f in range(H):
        if f in fd:
            counts[f] = fd[f]["cnt"]
            pos += [line * TOKENS + p for line, p in fd[f]["pos"]]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    masks, sens, spec = [], [], []
    for f, targets in pairs:
        masks.append(np.array([[any(t in tok for t in targets) for tok in row] for row in tokens], dtype=bool))
        with contextlib.redirect_stdout(io.StringIO()):
            sens.append(ins.check_sensitivity(fa, tokens, targets, f))
            spec.append(ins.check_specificity(fd, tokens, targets, f))
    assert spec[2] == 0.0 and masks[2].any()
    meta = {"lines": LINES, "tokens": TOKENS, "D": D, "H": H, "dead": DEAD, "torch": torch.__version__,
            "pairs": [[int(f), t] for f, t in pairs]}
    path = OUT / "inspector_overview.npz"
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        feature_activations=fa_np, counts=counts, offsets=offsets, positions=np.asarray(pos, np.int64),
                        tokens=np.array(tokens), match_masks=np.stack(masks), pair_features=np.array([f for f, _ in pairs], np.int64),
                        sensitivity=np.array(sens, np.float64), specificity=np.array(spec, np.float64))
    print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  {len(fd)} of {H} features won  pairs {meta['pairs']}  "
          f"sensitivity {sens}  specificity {spec}")


if __name__ == "__main__":
    main()
