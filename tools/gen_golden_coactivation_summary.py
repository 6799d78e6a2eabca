#!/usr/bin/env python3
"""Generate tests/golden/coactivation_summary_*.npz by running the REFERENCE's own summary functions (container-only).

Masks come from the portable recipes of tests/coactivation_partners_util.py; the matrix the reference receives is
``oracle.activation_stats(mask)[1]``.  scripts/analysis/summarize_stats.py is loaded by file path with the stub modules
of tools/gen_golden_token_overlap.py.  Its ``summarize_activation_counts``, ``count_below_threshold`` and
``average_coactivating_features`` run overall, per level (rows restricted to the level, partners over all features, as
its main() does) and on the recipe's extra ``row_mask``; the per-feature partner count is its
``average_coactivating_features`` with a one-hot ``row_mask`` (the mean of one element is the count itself, 0.0 for an
inactive feature).  Only data is written: the recipe, the mask packed to bytes, and those results.

Every case is checked here for what it is meant to exercise, so that a fixture cannot quietly stop exercising it.

Run:  python tools/gen_golden_coactivation_summary.py        (needs the reference checkout; CPU only, seconds)
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

import coactivation_partners_util as U  # noqa: E402
import oracle  # noqa: E402
from gen_golden_token_overlap import load_summarize_stats  # noqa: E402

OUT = ROOT / "tests" / "golden"


def one_hot(H, f):
    m = torch.zeros(H, dtype=torch.bool)
    m[f] = True
    return m


def main():
    ref = load_summarize_stats()
    OUT.mkdir(parents=True, exist_ok=True)
    for name, recipe in U.RECIPES.items():
        H, sizes, threshold = recipe["H"], recipe["sizes"], recipe["threshold"]
        mask = U.summary_mask(recipe)
        assert mask.shape == (recipe["B"], H) and H <= 192 and recipe["B"] <= 256 and sum(sizes) == H, name
        counts_np, coact_np = oracle.activation_stats(mask)
        act, coact = torch.from_numpy(counts_np), torch.from_numpy(coact_np)

        per_feature = np.array([ref.average_coactivating_features(coact, act, row_mask=one_hot(H, f)) for f in range(H)])
        assert (per_feature == np.round(per_feature)).all(), name
        per_feature = per_feature.astype(np.int64)
        assert (per_feature[counts_np == 0] == 0).all(), name
        assert per_feature.sum() < 2 ** 24 and counts_np.sum() < 2 ** 24, name

        def block(sl):
            row_mask = torch.zeros(H, dtype=torch.bool)
            row_mask[sl] = True
            return (ref.summarize_activation_counts(act[sl]), ref.count_below_threshold(act[sl], threshold),
                    ref.average_coactivating_features(coact, act, row_mask=row_mask))

        overall = (ref.summarize_activation_counts(act), ref.count_below_threshold(act, threshold),
                   ref.average_coactivating_features(coact, act))
        levels = [block(sl) for sl in U.level_slices(sizes)]
        row_mask = np.zeros(H, bool)
        row_mask[recipe["row_mask"]] = True
        selected = ref.average_coactivating_features(coact, act, row_mask=torch.from_numpy(row_mask))

        # coverage conditions
        active = counts_np > 0
        if name == "levels3":
            assert len(sizes) == 3 and (~active).any(), name
            f = recipe["lonely"]
            assert active[f] and per_feature[f] == 0, f"{name}: no active feature without partners"
            few = [int(active[sl].sum()) for sl in U.level_slices(sizes)]
            assert 0 < min(few) <= 4, f"{name}: no level with few active features: {few}"
            assert all(lv[2] > 0 for lv in levels) and overall[1] > int((~active).sum()), name
            U.check_density(coact_np[np.ix_(active, active)] > 0)
        if name == "single":
            assert len(sizes) == 1 and levels[0] == overall and overall[2] > 0, name
        if name == "nothing_active":
            assert not active.any() and overall[2] == 0.0 and all(lv[2] == 0.0 for lv in levels) and selected == 0.0, name
        if name == "dead_selection":
            assert active.any() and not active[row_mask].any() and selected == 0.0 and overall[2] > 0, name

        arrays = dict(mask=np.packbits(mask, axis=1, bitorder="little"), activation_counts=counts_np,
                      level_sizes=np.array(sizes, dtype=np.int64), threshold=np.int64(threshold),
                      partner_counts=per_feature, row_mask=row_mask,
                      mean_activation_count=np.array([overall[0]] + [lv[0] for lv in levels], dtype=np.float64),
                      below_threshold=np.array([overall[1]] + [lv[1] for lv in levels], dtype=np.int64),
                      avg_coactivating_features=np.array([overall[2]] + [lv[2] for lv in levels], dtype=np.float64),
                      avg_coactivating_selected=np.float64(selected))
        path = OUT / f"{U.GOLDEN_PREFIX}{name}.npz"
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8), **arrays)
        print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  active {int(active.sum())}/{H}  "
              f"avg partners {overall[2]:.3f}  levels {[round(lv[2], 3) for lv in levels]}")


if __name__ == "__main__":
    main()
