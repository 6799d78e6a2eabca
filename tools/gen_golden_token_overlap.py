#!/usr/bin/env python3
"""Generate tests/golden/token_overlap_*.npz by running the REFERENCE's own token-overlap comparison (container-only).

Token lists come from the portable recipes of tests/token_overlap_util.py.  scripts/analysis/summarize_stats.py is
loaded by file path with stub modules registered for the imports it cannot resolve (`sae_inference_framework`,
`SAEs.*`: only `get_level_sizes` uses them, which is not called).  Its `_topk_token_set` and `jaccard_between_saes` run
on the lists; only data is written: the recipe, the reference's sets (padded, sorted), the multiset of its scores as
(inter, union, count) triples, its pair count, its `nlargest` means and the fp64 `fsum` mean of its scores.

Every case is checked here for what it is meant to exercise, so that a fixture cannot quietly stop exercising it.

Run:  python tools/gen_golden_token_overlap.py        (needs the reference checkout; CPU only, seconds)
"""
from __future__ import annotations

import importlib.util
import json
import math
import sys
import types
from collections import Counter
from heapq import nlargest
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import token_overlap_util as U  # noqa: E402
from ref_loader import REF_ROOT  # noqa: E402

OUT = ROOT / "tests" / "golden"
TOPS = (10, 100, 1000, 10000)


def load_summarize_stats():
    stubs = {"sae_inference_framework": {"load_sae": None}, "SAEs": {},
             "SAEs.quantized_matryoshka_SAE": {"QuantizedMatryoshkaSAE": type("QuantizedMatryoshkaSAE", (), {})},
             "SAEs.residual_quantized_matryoshka_SAE": {"ResidualQuantizedSAE": type("ResidualQuantizedSAE", (), {})}}
    saved = {name: sys.modules.get(name) for name in stubs}
    for name, attrs in stubs.items():
        m = types.ModuleType(name)
        m.__path__ = []
        for key, value in attrs.items():
            setattr(m, key, value)
        sys.modules[name] = m
    try:
        path = REF_ROOT / "scripts" / "analysis" / "summarize_stats.py"
        spec = importlib.util.spec_from_file_location("ref_summarize_stats", str(path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name, old in saved.items():
            if old is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = old
    return mod


def padded_sets(ref, lists, act, k):
    out = np.full((len(lists), k), -1, dtype=np.int64)
    for i, lst in enumerate(lists):
        if act[i] > 0:
            s = sorted(ref._topk_token_set(lst, k))
            out[i, :len(s)] = s
    return out


def has_boundary_tie(lists, act, k):
    for lst, a in zip(lists, act):
        c = [n for _, n in Counter(lst).most_common()]
        if a > 0 and len(c) > k and c[k - 1] == c[k]:
            return True
    return False


def main():
    ref = load_summarize_stats()
    OUT.mkdir(parents=True, exist_ok=True)
    empty_share = {}
    for name, recipe in U.RECIPES.items():
        k, V = recipe["k"], recipe["V"]
        la, aa, lb, ab = U.token_lists(recipe)
        stats_a = {"tokens_per_feature": la, "activation_counts": torch.from_numpy(aa)}
        stats_b = {"tokens_per_feature": lb, "activation_counts": torch.from_numpy(ab)}
        scores = ref.jaccard_between_saes(stats_a, stats_b, k)
        sets_a, sets_b = padded_sets(ref, la, aa, k), padded_sets(ref, lb, ab, k)
        size_a, size_b = (sets_a >= 0).sum(1), (sets_b >= 0).sum(1)

        # the formulation: the reference's scores are the scores of the (inter, union) histogram of its own sets
        hist = U.hist_numpy(U.membership(sets_a, V), size_a, U.membership(sets_b, V), size_b, k)
        ii, uu = np.nonzero(hist)
        triples = np.stack([ii, uu, hist[ii, uu]], axis=1).astype(np.int64)
        expanded = [(i / u if i else 0.0) for i, u, c in triples.tolist() for _ in range(c)]
        assert sorted(scores) == sorted(expanded), name
        assert len(scores) == int((size_a > 0).sum()) * int((size_b > 0).sum()), name

        # coverage conditions
        assert recipe["Na"] != recipe["Nb"], name
        for lists, act, size in ((la, aa, size_a), (lb, ab, size_b)):
            assert any(a == 0 and not t for a, t in zip(act, lists)), f"{name}: no never-active feature"
            assert any(a == 0 and t for a, t in zip(act, lists)), f"{name}: no inactive feature with a list"
            assert (size == 0).any() and ((size > 0) & (size < k)).any() and (size == k).any(), f"{name}: set sizes"
            assert has_boundary_tie(lists, act, k), f"{name}: no tie at the k-th token"
        assert hist[1:].sum() and any(i == u for i, u, _ in triples.tolist() if i), f"{name}: no identical pair"
        assert hist[0].sum() > 0, f"{name}: no empty intersection"
        empty_share[name] = hist[0].sum() / len(scores)

        tops = {n: nlargest(n, scores) for n in TOPS}
        arrays = dict(sets_a=sets_a.astype(np.int32), sets_b=sets_b.astype(np.int32), triples=triples,
                      n_pairs=np.int64(len(scores)), top_n=np.array(TOPS, dtype=np.int64),
                      top_used=np.array([len(tops[n]) for n in TOPS], dtype=np.int64),
                      top_mean=np.array([float(sum(tops[n]) / len(tops[n])) for n in TOPS], dtype=np.float64),
                      top_scores=np.array(tops[TOPS[-1]], dtype=np.float64),
                      mean=np.float64(math.fsum(scores) / len(scores)))
        path = OUT / f"{name}.npz"
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8), **arrays)
        print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  pairs {len(scores)}  "
              f"empty {empty_share[name]:.3f}  bins {len(triples)}")
    assert any(0.2 <= s <= 0.8 for s in empty_share.values()), f"no case with 20-80 % empty intersections: {empty_share}"


if __name__ == "__main__":
    main()
