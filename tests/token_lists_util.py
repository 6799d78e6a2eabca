"""The definition that the token-list tests restate (dynamic_analysis.py:283-306): over the concatenated batches,
tokens_per_feature[f] = flat_tok[np.nonzero(mask[:, f])[0]], and the CSR form of that."""
import numpy as np


def row_tokens(n, start=0):
    """Non-monotonic token ids of rows start .. start + n - 1, so that a misordered list shows."""
    return ((np.arange(start, start + n, dtype=np.int64) * 7919) % 50257).astype(np.int32)


def restate(mask, flat_tok):
    """-> (offsets int64 [H + 1], tokens int32 [nnz]) of a bool mask [rows, H] and the rows' tokens."""
    mask = np.asarray(mask, bool)
    lists = [np.asarray(flat_tok)[np.nonzero(mask[:, f])[0]] for f in range(mask.shape[1])]
    offsets = np.zeros(mask.shape[1] + 1, np.int64)
    np.cumsum([len(t) for t in lists], out=offsets[1:])
    tokens = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return offsets, tokens


def pack(bits):
    """bool [B, 32 w] -> int32 [B, w], bit j of word w = column 32 w + j."""
    bits = np.asarray(bits, bool)
    if bits.shape[0] == 0:
        return np.zeros((0, bits.shape[1] // 32), np.int32)
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view(np.int32)
