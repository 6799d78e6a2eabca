"""``torch.ops.qsae.*``: the kernels of libqsae_hip.so registered with the PyTorch dispatcher.

The reference's compute is a sequence of ATen ops (``F.linear``, ``torch.topk``, ``scatter_``, ``matmul``: sae/binary.py:24-47,
91-103, sae/baseline.py:17-40, sae/ternary.py:41-52, sae/quantized_matryoshka.py:47-143); here every kernel entry point of the
C ABI (include/qsae.h) is a dispatcher op of namespace ``qsae`` with a fake (meta) implementation, so the module classes'
forwards are visible to ``torch.compile`` / ``torch.export`` as graph nodes instead of opaque ctypes calls.  Two layers:

* kernel level -- ``torch.ops.qsae.encode_dense``, ``.encode_topk_prefilter``, ``.binary_forward_prefilter``,
  ``.decode_binary_sparse`` ...: thin registrations over ``quantizedsae_amd.ops`` (which binds the C ABI with ctypes; torch only
  supplies device memory and the current stream).  The module classes call these (through the same-named Python functions of
  this module, which keep the keyword defaults of ``ops.py``).
* model level -- ``torch.ops.qsae.binary_sae_forward`` / ``baseline_sae_forward`` / ``ternary_sae_forward`` /
  ``matryoshka_sae_forward`` / ``residual_sae_forward``: one node per ``forward()``, used by the module classes while they are
  being traced (``torch.compiler.is_compiling()``).  The Python around the kernels (derived-weight caches keyed on parameter
  versions, path selection by shape, the host read of the flagged-row count) is not traceable and does not need to be: the node
  takes the input batch and the parameters and finds its module through a process-local handle.

CUDA (ROCm) tensors only: there is no CPU implementation to register, the ops raise on CPU tensors like ``ops.py`` does.
"""
from __future__ import annotations

import inspect
import weakref
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import ops as _ops
from .ops import ACT_NONE, ACT_RELU, ACT_SIGMOID  # noqa: F401

_NS = "qsae"


def _op(name, mutates=()):
    return torch.library.custom_op(f"{_NS}::{name}", mutates_args=mutates)


def _i32(shape, like):
    return torch.empty(shape, dtype=torch.int32, device=like.device)


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _host_count():
    return torch.empty((), dtype=torch.int64)


# ---- encoder -------------------------------------------------------------------------------------------------------
@_op("kperm_rows")
def _kperm_rows(src: Tensor) -> Tensor:
    return _ops.kperm_rows(src)


@_kperm_rows.register_fake
def _(src):
    return _f32(src.shape, src)


@_op("encode_dense")
def _encode_dense(x: Tensor, W: Tensor, bias: Optional[Tensor], act: int, kperm: bool) -> Tensor:
    return _ops.encode_dense(x, W, bias, act, kperm=kperm)


@_encode_dense.register_fake
def _(x, W, bias, act, kperm):
    return _f32((x.shape[0], W.shape[0]), x)


@_op("emu_pack_w")
def _emu_pack_w(W: Tensor) -> Tuple[Tensor, Tensor]:
    return _ops.emu_pack_w(W)


@_emu_pack_w.register_fake
def _(W):
    return torch.empty((W.shape[0], 3 * W.shape[1]), dtype=torch.float16, device=W.device), _f32((2,), W)


@_op("encode_dense_emu")
def _encode_dense_emu(x: Tensor, Wc: Tensor, meta2: Tensor, bias: Optional[Tensor], act: int) -> Tensor:
    return _ops.encode_dense_emu(x, Wc, meta2, bias, act)


@_encode_dense_emu.register_fake
def _(x, Wc, meta2, bias, act):
    return _f32((x.shape[0], Wc.shape[0]), x)


@_op("encode_bits")
def _encode_bits(x: Tensor, W: Tensor, bias: Optional[Tensor]) -> Tensor:
    return _ops.encode_bits(x, W, bias)


@_encode_bits.register_fake
def _(x, W, bias):
    return _i32((x.shape[0], (W.shape[0] + 31) // 32), x)


def _register_bits_fp16(kind):
    """torch.ops.qsae.encode_bits_<kind> -> (z bits, host count of the rows that took the exact kernel), and its fake."""
    fn = getattr(_ops, f"encode_bits_{kind}")

    @_op(f"encode_bits_{kind}")
    def op(x: Tensor, W: Tensor, bias: Optional[Tensor], Wq: Tensor, meta: Tensor) -> Tuple[Tensor, Tensor]:
        z, flagged = fn(x, W, bias, Wq, meta)
        return z, torch.tensor(flagged, dtype=torch.int64)

    @op.register_fake
    def _(x, W, bias, Wq, meta):
        return _i32((x.shape[0], (W.shape[0] + 31) // 32), x), _host_count()


_register_bits_fp16("prefilter")
_register_bits_fp16("band")


@_op("topk_rows", mutates=("latent",))
def _topk_rows(latent: Tensor, k: int, zero_rest: bool) -> Tuple[Tensor, Tensor]:
    return _ops.topk_rows(latent, k, zero_rest)


@_topk_rows.register_fake
def _(latent, k, zero_rest):
    return _i32((latent.shape[0], k), latent), _f32((latent.shape[0], k), latent)


@_op("encode_topk")
def _encode_topk(x: Tensor, W: Tensor, bias: Optional[Tensor], k: int, kperm: bool) -> Tuple[Tensor, Tensor]:
    return _ops.encode_topk(x, W, bias, k, kperm=kperm)


@_encode_topk.register_fake
def _(x, W, bias, k, kperm):
    return _i32((x.shape[0], k), x), _f32((x.shape[0], k), x)


@_op("encode_topk_latent")
def _encode_topk_latent(x: Tensor, W: Tensor, bias: Optional[Tensor], k: int, kperm: bool) -> Tuple[Tensor, Tensor, Tensor]:
    return _ops.encode_topk_latent(x, W, bias, k, kperm=kperm)


@_encode_topk_latent.register_fake
def _(x, W, bias, k, kperm):
    return _i32((x.shape[0], k), x), _f32((x.shape[0], k), x), _f32((x.shape[0], W.shape[0]), x)


@_op("prefilter_pack_w")
def _prefilter_pack_w(W: Tensor, bias: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    return _ops.prefilter_pack_w(W, bias)


@_prefilter_pack_w.register_fake
def _(W, bias):
    return torch.empty(W.shape, dtype=torch.float16, device=W.device), _f32((4,), W)


def _dense_or_empty(dense, like, H):
    return dense if dense is not None else _f32((0, H), like)


@_op("encode_topk_prefilter")
def _encode_topk_prefilter(x: Tensor, W: Tensor, bias: Optional[Tensor], Wq: Tensor, meta: Tensor, k: int, want_dense: bool,
                           spec_rows: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    info = {}
    idx, val, dense = _ops.encode_topk_prefilter(x, W, bias, Wq, meta, k, want_dense=want_dense, spec_rows=spec_rows, info=info)
    return idx, val, _dense_or_empty(dense, x, W.shape[0]), torch.tensor(info["flagged_rows"], dtype=torch.int64)


@_encode_topk_prefilter.register_fake
def _(x, W, bias, Wq, meta, k, want_dense, spec_rows):
    B, H = x.shape[0], W.shape[0]
    return _i32((B, k), x), _f32((B, k), x), _f32((B if want_dense else 0, H), x), _host_count()


@_op("binary_forward_prefilter")
def _binary_forward_prefilter(x: Tensor, W: Tensor, bias: Optional[Tensor], Wq: Tensor, meta: Tensor, k: int, packed: Tensor,
                              n_bits: int, step: float, dec_bias: Optional[Tensor], want_dense: bool,
                              spec_rows: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    info = {}
    idx, val, dense, recon = _ops.binary_forward_prefilter(x, W, bias, Wq, meta, k, packed, n_bits, step, dec_bias,
                                                           want_dense=want_dense, spec_rows=spec_rows, info=info)
    return idx, val, _dense_or_empty(dense, x, W.shape[0]), recon, torch.tensor(info["flagged_rows"], dtype=torch.int64)


@_binary_forward_prefilter.register_fake
def _(x, W, bias, Wq, meta, k, packed, n_bits, step, dec_bias, want_dense, spec_rows):
    B, H = x.shape[0], W.shape[0]
    return _i32((B, k), x), _f32((B, k), x), _f32((B if want_dense else 0, H), x), _f32((B, x.shape[1]), x), _host_count()


@_op("table_forward_prefilter")
def _table_forward_prefilter(x: Tensor, W: Tensor, bias: Optional[Tensor], Wq: Tensor, meta: Tensor, k: int, table: Tensor,
                             scale: float, dec_bias: Optional[Tensor], want_dense: bool,
                             spec_rows: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    info = {}
    idx, val, dense, recon = _ops.table_forward_prefilter(x, W, bias, Wq, meta, k, table, scale, dec_bias,
                                                          want_dense=want_dense, spec_rows=spec_rows, info=info)
    return idx, val, _dense_or_empty(dense, x, W.shape[0]), recon, torch.tensor(info["flagged_rows"], dtype=torch.int64)


@_table_forward_prefilter.register_fake
def _(x, W, bias, Wq, meta, k, table, scale, dec_bias, want_dense, spec_rows):
    B, H = x.shape[0], W.shape[0]
    return _i32((B, k), x), _f32((B, k), x), _f32((B if want_dense else 0, H), x), _f32((B, x.shape[1]), x), _host_count()


@_op("densify")
def _densify(idx: Tensor, val: Tensor, H: int) -> Tensor:
    return _ops.densify(idx, val, H)


@_densify.register_fake
def _(idx, val, H):
    return _f32((idx.shape[0], H), idx)


# ---- BinarySAE dictionary ------------------------------------------------------------------------------------------
@_op("pack_binary")
def _pack_binary(logits: Tensor, D: int, n_bits: int) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (packed uint8 [H, row_bytes], polarize_sum float64 0-d, soft_gap float32 0-d)"""
    return _ops.pack_binary(logits, D, n_bits, want_polarize=True, want_soft_gap=True)


@_pack_binary.register_fake
def _(logits, D, n_bits):
    fw = 1 if n_bits <= 1 else 2 if n_bits <= 2 else 4 if n_bits <= 4 else 8
    row_bytes = ((D * fw + 31) // 32) * 4
    return (torch.empty((logits.shape[0], row_bytes), dtype=torch.uint8, device=logits.device),
            torch.empty((), dtype=torch.float64, device=logits.device), _f32((), logits))


@_op("unpack_binary")
def _unpack_binary(packed: Tensor, D: int, n_bits: int) -> Tensor:
    return _ops.unpack_binary(packed, D, n_bits)


@_unpack_binary.register_fake
def _(packed, D, n_bits):
    return _f32((packed.shape[0], D), packed)


@_op("binary_soft_table")
def _binary_soft_table(logits: Tensor, D: int, n_bits: int) -> Tensor:
    return _ops.binary_soft_table(logits, D, n_bits)


@_binary_soft_table.register_fake
def _(logits, D, n_bits):
    return _f32((logits.shape[0], D), logits)


@_op("decode_binary_sparse")
def _decode_binary_sparse(idx: Tensor, val: Tensor, packed: Tensor, D: int, n_bits: int, step: float,
                          bias: Optional[Tensor]) -> Tensor:
    return _ops.decode_binary_sparse(idx, val, packed, D, n_bits, step, bias)


@_decode_binary_sparse.register_fake
def _(idx, val, packed, D, n_bits, step, bias):
    return _f32((idx.shape[0], D), idx)


@_op("decode_table_sparse")
def _decode_table_sparse(idx: Tensor, val: Tensor, table: Tensor, scale: float, bias: Optional[Tensor]) -> Tensor:
    return _ops.decode_table_sparse(idx, val, table, scale, bias)


@_decode_table_sparse.register_fake
def _(idx, val, table, scale, bias):
    return _f32((idx.shape[0], table.shape[1]), idx)


# ---- ternary / matryoshka --------------------------------------------------------------------------------------------
@_op("pack_ternary")
def _pack_ternary(w: Tensor) -> Tensor:
    return _ops.pack_ternary(w)


@_pack_ternary.register_fake
def _(w):
    return _i32((w.shape[0], (w.shape[1] + 15) // 16), w)


@_op("decode_ternary_dense")
def _decode_ternary_dense(h: Tensor, codes: Tensor, D: int) -> Tensor:
    return _ops.decode_ternary_dense(h, codes, D)


@_decode_ternary_dense.register_fake
def _(h, codes, D):
    return _f32((h.shape[0], D), h)


@_op("pack_matryoshka")
def _pack_matryoshka(w: Tensor, wm: Tensor, n_bits: int, abs_range: float, sizes: Optional[List[int]]) -> Tuple[Tensor, Tensor]:
    return _ops.pack_matryoshka(w, wm, n_bits, abs_range, sizes)


@_pack_matryoshka.register_fake
def _(w, wm, n_bits, abs_range, sizes):
    return _i32((w.shape[1], (w.shape[0] + 15) // 16), w), _f32((w.shape[0],), w)


@_op("pack_matryoshka_rows")
def _pack_matryoshka_rows(w: Tensor, wm: Tensor) -> Tensor:
    return _ops.pack_matryoshka_rows(w, wm)


@_pack_matryoshka_rows.register_fake
def _(w, wm):
    return _i32((w.shape[0], (w.shape[1] + 7) // 8), w)


@_op("decode_matryoshka")
def _decode_matryoshka(zbits: Tensor, H: int, D: int, n_bits: int, codes: Tensor, scale: Tensor, bias: Optional[Tensor],
                       allow_bias: bool, sizes: Optional[List[int]], sparse: bool) -> Tuple[Tensor, Tensor]:
    """sparse: codes = the hidden-major dictionary (pack_matryoshka_rows), active units only; same outputs."""
    fn = _ops.decode_matryoshka_sparse if sparse else _ops.decode_matryoshka
    return fn(zbits, H, D, n_bits, codes, scale, bias, allow_bias, sizes)


@_decode_matryoshka.register_fake
def _(zbits, H, D, n_bits, codes, scale, bias, allow_bias, sizes, sparse):
    return _f32((n_bits, zbits.shape[0], D), zbits), torch.empty((n_bits,), dtype=torch.int64, device=zbits.device)


@_op("expand_codes_bf16")
def _expand_codes_bf16(codes: Tensor, D: int, H: int) -> Tensor:
    return _ops.expand_codes_bf16(codes, D, H)


@_expand_codes_bf16.register_fake
def _(codes, D, H):
    return torch.empty((H * D,), dtype=torch.bfloat16, device=codes.device)


@_op("decode_ternary_dense_split")
def _decode_ternary_dense_split(h: Tensor, tq: Tensor, D: int) -> Tensor:
    return _ops.decode_ternary_dense_split(h, tq, D)


@_decode_ternary_dense_split.register_fake
def _(h, tq, D):
    return _f32((h.shape[0], D), h)


@_op("split_scale_bf16")
def _split_scale_bf16(scale: Tensor) -> Tensor:
    return _ops.split_scale_bf16(scale)


@_split_scale_bf16.register_fake
def _(scale):
    return torch.empty((3, scale.shape[0]), dtype=torch.bfloat16, device=scale.device)


@_op("decode_matryoshka_split")
def _decode_matryoshka_split(zbits: Tensor, H: int, D: int, n_bits: int, tq: Tensor, s3: Tensor, bias: Optional[Tensor],
                             allow_bias: bool, sizes: Optional[List[int]]) -> Tuple[Tensor, Tensor]:
    return _ops.decode_matryoshka_split(zbits, H, D, n_bits, tq, s3, bias, allow_bias, sizes)


@_decode_matryoshka_split.register_fake
def _(zbits, H, D, n_bits, tq, s3, bias, allow_bias, sizes):
    return _f32((n_bits, zbits.shape[0], D), zbits), torch.empty((n_bits,), dtype=torch.int64, device=zbits.device)


@_op("pack_bits_gt")
def _pack_bits_gt(dense: Tensor, thr: float) -> Tensor:
    return _ops.pack_bits_gt(dense, thr)


@_pack_bits_gt.register_fake
def _(dense, thr):
    return _i32((dense.shape[0], (dense.shape[1] + 31) // 32), dense)


# ---- elementwise steps, metric, statistics ---------------------------------------------------------------------------
@_op("residual_update")
def _residual_update(residual: Tensor, recon: Tensor, scale: float) -> Tensor:
    return _ops.residual_update(residual, recon, scale)


@_residual_update.register_fake
def _(residual, recon, scale):
    return _f32(residual.shape, residual)


@_op("threshold_ge")
def _threshold_ge(pre: Tensor, cutoff: float) -> Tensor:
    return _ops.threshold_ge(pre, cutoff)


@_threshold_ge.register_fake
def _(pre, cutoff):
    return _f32(pre.shape, pre)


@_op("scale_bias_rows")
def _scale_bias_rows(acc: Tensor, scale: float, bias: Optional[Tensor]) -> Tensor:
    return _ops.scale_bias_rows(acc, scale, bias)


@_scale_bias_rows.register_fake
def _(acc, scale, bias):
    return _f32(acc.shape, acc)


@_op("sq_err_sum", mutates=("acc",))
def _sq_err_sum(recon: Tensor, x: Tensor, acc: Tensor) -> None:
    _ops.sq_err_sum(recon, x, acc)


@_op("activation_counts", mutates=("counts",))
def _activation_counts(idx: Tensor, val: Optional[Tensor], counts: Tensor) -> None:
    _ops.activation_counts(idx, val, counts.shape[0], counts)


@_op("activation_counts_bits", mutates=("counts",))
def _activation_counts_bits(zbits: Tensor, counts: Tensor) -> None:
    _ops.activation_counts_bits(zbits, counts)


@_op("coactivation_sparse", mutates=("coact",))
def _coactivation_sparse(idx: Tensor, val: Optional[Tensor], coact: Tensor) -> None:
    _ops.coactivation_sparse(idx, val, coact.shape[0], coact)


@_op("coactivation_bits", mutates=("coact",))
def _coactivation_bits(zbits: Tensor, index: Optional[Tensor], coact: Tensor) -> None:
    _ops.coactivation_bits(zbits, coact.shape[0], index, coact)


@_coactivation_bits.register_fake
def _(zbits, index, coact):
    return None


@_op("coactivation_partners_bits", mutates=("partners",))
def _coactivation_partners_bits(zbits: Tensor, index: Optional[Tensor], partners: Tensor) -> None:
    _ops.coactivation_partners_bits(zbits, index, partners)


@_coactivation_partners_bits.register_fake
def _(zbits, index, partners):
    return None


@_op("coactivation_partners_sparse", mutates=("partners",))
def _coactivation_partners_sparse(idx: Tensor, val: Optional[Tensor], H: int, partners: Tensor) -> None:
    _ops.coactivation_partners_sparse(idx, val, H, partners)


@_coactivation_partners_sparse.register_fake
def _(idx, val, H, partners):
    return None


@_op("coactivation_partner_counts")
def _coactivation_partner_counts(partners: Tensor, H: int, index: Optional[Tensor]) -> Tensor:
    return _ops.coactivation_partner_counts(partners, H, index)


@_coactivation_partner_counts.register_fake
def _(partners, H, index):
    return torch.empty((H,), dtype=torch.int64, device=partners.device)


@_op("coactivation_partner_counts_dense")
def _coactivation_partner_counts_dense(coact: Tensor, row0: int) -> Tensor:
    return _ops.coactivation_partner_counts_dense(coact, row0)


@_coactivation_partner_counts_dense.register_fake
def _(coact, row0):
    return torch.empty((coact.shape[0],), dtype=torch.int64, device=coact.device)


@_op("token_overlap_hist", mutates=("hist",))
def _token_overlap_hist(asets: Tensor, asize: Tensor, bsets: Tensor, bsize: Tensor, V: int, k: int, hist: Tensor) -> None:
    _ops.token_overlap_hist(asets, asize, bsets, bsize, V, k, hist)


@_token_overlap_hist.register_fake
def _(asets, asize, bsets, bsize, V, k, hist):
    return None


@_op("token_lists_count")
def _token_lists_count(idx: Tensor, val: Optional[Tensor], H: int) -> Tuple[Tensor, Tensor]:
    return _ops.token_lists_count(idx, val, H)


@_op("token_lists_count_bits")
def _token_lists_count_bits(zbits: Tensor, index: Optional[Tensor], H: int) -> Tuple[Tensor, Tensor]:
    return _ops.token_lists_count_bits(zbits, H, index)


def _token_lists_count_fake(rows, H, like):
    return (torch.empty((H + 1,), dtype=torch.int64, device=like.device),
            torch.empty((_ops.token_lists_workspace_bytes(rows, H),), dtype=torch.uint8, device=like.device))


@_token_lists_count.register_fake
def _(idx, val, H):
    return _token_lists_count_fake(idx.shape[0], H, idx)


@_token_lists_count_bits.register_fake
def _(zbits, index, H):
    return _token_lists_count_fake(zbits.shape[0], H, zbits)


@_op("token_lists_fill")
def _token_lists_fill(workspace: Tensor, offsets: Tensor, row_tokens: Tensor, n_entries: int) -> Tensor:
    return _ops.token_lists_fill(workspace, offsets, row_tokens, n_entries)


@_token_lists_fill.register_fake
def _(workspace, offsets, row_tokens, n_entries):
    return _i32((n_entries,), offsets)


@_op("token_lists_regroup")
def _token_lists_regroup(batch_offsets: Tensor, segments: Tensor) -> Tuple[Tensor, Tensor]:
    return _ops.token_lists_regroup(batch_offsets, segments)


@_token_lists_regroup.register_fake
def _(batch_offsets, segments):
    return (torch.empty((batch_offsets.shape[1],), dtype=torch.int64, device=batch_offsets.device),
            _i32(segments.shape, segments))


@_op("top_examples_compact", mutates=("keys",))
def _top_examples_compact(idx: Tensor, val: Optional[Tensor], floor: float, base: int, keys: Tensor) -> None:
    _ops.top_examples_compact(idx, val, floor, base, keys)


@_top_examples_compact.register_fake
def _(idx, val, floor, base, keys):
    return None


@_op("top_examples_dense", mutates=("keys",))
def _top_examples_dense(latent: Tensor, floor: float, base: int, keys: Tensor) -> None:
    _ops.top_examples_dense(latent, floor, base, keys)


@_top_examples_dense.register_fake
def _(latent, floor, base, keys):
    return None


@_op("top_examples_decode")
def _top_examples_decode(keys: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    return _ops.top_examples_decode(keys)


@_top_examples_decode.register_fake
def _(keys):
    return (_f32(keys.shape, keys), torch.empty(keys.shape, dtype=torch.int64, device=keys.device),
            _i32((keys.shape[0],), keys))


@_op("quantization_error")
def _quantization_error(logits: Tensor, D: int, n_bits: int, step: float, margin_logit: float) -> Tuple[Tensor, Tensor]:
    """-> (result fp64 [48], unit_err_sq fp64 [H]) as in qsae_quantization_error"""
    return _ops.quantization_error(logits, D, n_bits, step, margin_logit)


@_quantization_error.register_fake
def _(logits, D, n_bits, step, margin_logit):
    f64 = dict(dtype=torch.float64, device=logits.device)
    return torch.empty((_ops.QUANT_ERROR_WORDS,), **f64), torch.empty((logits.shape[0],), **f64)


@_op("dataset_moments_add", mutates=("sums", "counts"))
def _dataset_moments_add(x: Tensor, recon: Optional[Tensor], group_rows: int, sums: Tensor, counts: Tensor) -> None:
    _ops.dataset_moments_add(x, recon, group_rows, sums, counts)


@_dataset_moments_add.register_fake
def _(x, recon, group_rows, sums, counts):
    return None


@_op("quantize_bits")
def _quantize_bits(x: Tensor, n_bits: int, scale_factor: float, signed: bool) -> Tensor:
    return _ops.quantize_bits(x, n_bits, scale_factor, signed)


@_quantize_bits.register_fake
def _(x, n_bits, scale_factor, signed):
    return _f32((x.shape[0], x.shape[1] * n_bits), x)


# ---- decoder dictionary comparison ------------------------------------------------------------------------------------
@_op("cosine_compare")
def _cosine_compare(A: Tensor, B: Optional[Tensor], thresholds: List[float], bins: int,
                    want_matrix: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (row_best [Ha], col_best [Hb] ([0] in self mode, B None), moments fp64 [2], extrema [2], counts [len(thresholds)],
    hist [bins], matrix [Ha, Hb] or [0, 0]); keys int64 as in qsae_cosine_compare"""
    return _ops.cosine_compare(A, B, thresholds, bins, want_matrix)


@_cosine_compare.register_fake
def _(A, B, thresholds, bins, want_matrix):
    Ha = A.shape[0]
    Hb = Ha if B is None else B.shape[0]
    i64 = dict(dtype=torch.int64, device=A.device)
    return (torch.empty((Ha,), **i64), torch.empty((0 if B is None else Hb,), **i64),
            torch.empty((2,), dtype=torch.float64, device=A.device), torch.empty((2,), **i64),
            torch.empty((len(thresholds),), **i64), torch.empty((bins,), **i64),
            _f32((Ha, Hb) if want_matrix else (0, 0), A))


@_op("nearest_atoms_i8")
def _nearest_atoms_i8(a: Tensor, b: Optional[Tensor], k: int, exclude_self: bool,
                      want_duplicates: bool) -> Tuple[Tensor, Tensor]:
    """-> (keys int64 [Na, k], duplicate_of int32 [Na] or [0]); keys as in qsae_nearest_atoms_i8"""
    keys, dup = _ops.nearest_atoms_i8(a, b, k, exclude_self, want_duplicates)
    return keys, (dup if dup is not None else _i32((0,), a))


@_nearest_atoms_i8.register_fake
def _(a, b, k, exclude_self, want_duplicates):
    return (torch.empty((a.shape[0], k), dtype=torch.int64, device=a.device),
            _i32((a.shape[0] if want_duplicates else 0,), a))


@_op("nearest_atoms_f32")
def _nearest_atoms_f32(a: Tensor, b: Optional[Tensor], k: int, exclude_self: bool) -> Tensor:
    """-> keys int64 [Na, k] as in qsae_nearest_atoms_f32"""
    return _ops.nearest_atoms_f32(a, b, k, exclude_self)


@_nearest_atoms_f32.register_fake
def _(a, b, k, exclude_self):
    return torch.empty((a.shape[0], k), dtype=torch.int64, device=a.device)


@_op("kmeans_assign")
def _kmeans_assign(atoms: Tensor, centers: Tensor, metric: str) -> Tensor:
    """-> keys int64 [N] as in qsae_kmeans_assign_f32"""
    return _ops.kmeans_assign(atoms, centers, metric)


@_kmeans_assign.register_fake
def _(atoms, centers, metric):
    return torch.empty((atoms.shape[0],), dtype=torch.int64, device=atoms.device)


@_op("kmeans_update")
def _kmeans_update(atoms: Tensor, labels: Tensor, centers_old: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (centers_new fp32 [C, D], counts int32 [C], stats fp64 [2]) as in qsae_kmeans_update_f32"""
    return _ops.kmeans_update(atoms, labels, centers_old)


@_kmeans_update.register_fake
def _(atoms, labels, centers_old):
    C = centers_old.shape[0]
    return (_f32((C, centers_old.shape[1]), atoms), _i32((C,), atoms),
            torch.empty((2,), dtype=torch.float64, device=atoms.device))


# ---- BinarySAE training ----------------------------------------------------------------------------------------------
@_op("binary_soft_table_polarize")
def _binary_soft_table_polarize(logits: Tensor, D: int, n_bits: int) -> Tuple[Tensor, Tensor]:
    """-> (soft table [H, D], polarize fp32 0-d), both on the device"""
    return _ops.binary_soft_table_polarize(logits, D, n_bits)


@_binary_soft_table_polarize.register_fake
def _(logits, D, n_bits):
    return _f32((logits.shape[0], D), logits), _f32((), logits)


@_op("train_csr")
def _train_csr(idx: Tensor, H: int) -> Tuple[Tensor, Tensor]:
    """-> (offsets int32 [H + 1], entries int32 [B k]): the top-k lists grouped by unit, ordered by row"""
    return _ops.train_csr(idx, H)


@_train_csr.register_fake
def _(idx, H):
    return _i32((H + 1,), idx), _i32((idx.shape[0] * idx.shape[1],), idx)


@_op("train_row_grad")
def _train_row_grad(idx: Tensor, table: Tensor, step: float, g_recon: Optional[Tensor], g_latent: Optional[Tensor],
                    W_enc: Optional[Tensor], want_dx: bool) -> Tuple[Tensor, Tensor]:
    """-> (gv [B, k], dx [B, D] ([0, D] when not wanted))"""
    gv, dx = _ops.train_row_grad(idx, table, step, g_recon, g_latent, W_enc, want_dx)
    return gv, (dx if dx is not None else _f32((0, table.shape[1]), idx))


@_train_row_grad.register_fake
def _(idx, table, step, g_recon, g_latent, W_enc, want_dx):
    return _f32(tuple(idx.shape), idx), _f32((idx.shape[0] if want_dx else 0, table.shape[1]), idx)


@_op("train_unit_grad")
def _train_unit_grad(offsets: Tensor, entries: Tensor, val: Tensor, gv: Tensor, x: Tensor, g_recon: Optional[Tensor],
                     logits: Tensor, n_bits: int, step: float, g_polarize: Optional[Tensor], want_encoder: bool,
                     want_logits: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (dW_enc [H, D], db_enc [H], dlogits [H, D n_bits]); an output not wanted has 0 rows"""
    dW, db, dl = _ops.train_unit_grad(offsets, entries, val, gv, x, g_recon, logits, n_bits, step, g_polarize,
                                      want_encoder, want_logits)
    D = x.shape[1]
    return (dW if dW is not None else _f32((0, D), x), db if db is not None else _f32((0,), x),
            dl if dl is not None else _f32((0, logits.shape[1]), x))


@_train_unit_grad.register_fake
def _(offsets, entries, val, gv, x, g_recon, logits, n_bits, step, g_polarize, want_encoder, want_logits):
    H, D = offsets.shape[0] - 1, x.shape[1]
    return (_f32((H if want_encoder else 0, D), x), _f32((H if want_encoder else 0,), x),
            _f32((H if want_logits else 0, logits.shape[1]), x))


@_op("train_col_sum")
def _train_col_sum(g: Tensor) -> Tensor:
    return _ops.train_col_sum(g)


@_train_col_sum.register_fake
def _(g):
    return _f32((g.shape[1],), g)


# ---- BaselineSparseAutoencoder training ---------------------------------------------------------------------------------
@_op("train_table_unit_grad")
def _train_table_unit_grad(offsets: Tensor, entries: Tensor, val: Tensor, gv: Tensor, x: Tensor, g_recon: Optional[Tensor],
                           want_encoder: bool, want_decoder: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (dW_enc [H, D], db_enc [H], dW_dec [D, H]); an output not wanted is empty ([0, D], [0], [D, 0])"""
    dW, db, dWd = _ops.train_table_unit_grad(offsets, entries, val, gv, x, g_recon, want_encoder, want_decoder)
    D = x.shape[1]
    return (dW if dW is not None else _f32((0, D), x), db if db is not None else _f32((0,), x),
            dWd if dWd is not None else _f32((D, 0), x))


@_train_table_unit_grad.register_fake
def _(offsets, entries, val, gv, x, g_recon, want_encoder, want_decoder):
    H, D = offsets.shape[0] - 1, x.shape[1]
    return (_f32((H if want_encoder else 0, D), x), _f32((H if want_encoder else 0,), x),
            _f32((D, H if want_decoder else 0), x))


@_op("normalize_columns_table", mutates=("W",))
def _normalize_columns_table(W: Tensor, want_table: bool) -> Tensor:
    """W [D, H] -> unit-norm columns in place; -> the normalised transpose [H, D] ([0, D] when not wanted)"""
    table = _ops.normalize_columns_table(W, want_table)
    return table if table is not None else _f32((0, W.shape[0]), W)


@_normalize_columns_table.register_fake
def _(W, want_table):
    return _f32((W.shape[1] if want_table else 0, W.shape[0]), W)


# ---- optimizer: in-place dispatcher ops, so that the version counters of what they write move and every PackedCache keyed
# on a stepped parameter rebuilds by itself ------------------------------------------------------------------------------------
@_op("adam_step", mutates=("p", "m", "v"))
def _adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, one_minus_b1: float, b2: float, one_minus_b2: float,
               bc2_sqrt: float, eps: float, step_size: float) -> None:
    _ops.adam_step(p, g, m, v, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size)


@_adam_step.register_fake
def _(p, g, m, v, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size):
    return None


@_op("adam_step_prefilter", mutates=("W", "mW", "vW", "bias", "mb", "vb", "Wq", "meta"))
def _adam_step_prefilter(W: Tensor, gW: Tensor, mW: Tensor, vW: Tensor, bias: Optional[Tensor], gb: Optional[Tensor],
                         mb: Optional[Tensor], vb: Optional[Tensor], one_minus_b1: float, b2: float, one_minus_b2: float,
                         bc2_sqrt: float, eps: float, step_size: float, Wq: Tensor, meta: Tensor) -> None:
    """Wq fp16 [H, D] and meta fp32 [4] receive the prefilter state of the updated W / bias"""
    _ops.adam_step_prefilter(W, gW, mW, vW, bias, gb, mb, vb, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size,
                             Wq, meta)


@_adam_step_prefilter.register_fake
def _(W, gW, mW, vW, bias, gb, mb, vb, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size, Wq, meta):
    return None


# ---- the recipe around the step (csrc/optim_recipe.hip): the written tensors are mutated arguments, as above ----------------
@_op("project_columns", mutates=("G",))
def _project_columns(W: Tensor, G: Tensor) -> None:
    """G [D, H] loses its component along every column of W [D, H], in place"""
    _ops.project_columns(W, G)


@_project_columns.register_fake
def _(W, G):
    return None


@_op("grad_norm", mutates=("coef", "report"))
def _grad_norm(tensors: List[Tensor], max_norm: float, coef: Tensor, report: Tensor) -> None:
    """coef fp32 [1] receives the clip coefficient of the joint norm, report int64 [4 + T] the sums behind it"""
    _ops.grad_norm(tensors, max_norm, coef, report)


@_grad_norm.register_fake
def _(tensors, max_norm, coef, report):
    return None


@_op("adam_step_clipped", mutates=("p", "m", "v", "ema"))
def _adam_step_clipped(p: Tensor, g: Tensor, m: Tensor, v: Tensor, one_minus_b1: float, b2: float, one_minus_b2: float,
                       bc2_sqrt: float, eps: float, step_size: float, coef: Optional[Tensor], ema: Optional[Tensor],
                       one_minus_decay: float) -> None:
    _ops.adam_step_clipped(p, g, m, v, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size, coef, ema, one_minus_decay)


@_adam_step_clipped.register_fake
def _(p, g, m, v, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size, coef, ema, one_minus_decay):
    return None


@_op("adam_step_prefilter_clipped", mutates=("W", "mW", "vW", "bias", "mb", "vb", "emaW", "emab", "Wq", "meta"))
def _adam_step_prefilter_clipped(W: Tensor, gW: Tensor, mW: Tensor, vW: Tensor, bias: Optional[Tensor], gb: Optional[Tensor],
                                 mb: Optional[Tensor], vb: Optional[Tensor], one_minus_b1: float, b2: float,
                                 one_minus_b2: float, bc2_sqrt: float, eps: float, step_size: float, coef: Optional[Tensor],
                                 emaW: Optional[Tensor], emab: Optional[Tensor], one_minus_decay: float, Wq: Tensor,
                                 meta: Tensor) -> None:
    """Wq fp16 [H, D] and meta fp32 [4] receive the prefilter state of the updated W / bias"""
    _ops.adam_step_prefilter_clipped(W, gW, mW, vW, bias, gb, mb, vb, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size,
                                     coef, emaW, emab, one_minus_decay, Wq, meta)


@_adam_step_prefilter_clipped.register_fake
def _(W, gW, mW, vW, bias, gb, mb, vb, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size, coef, emaW, emab,
      one_minus_decay, Wq, meta):
    return None


# ---- trainer: batch supply and loss (csrc/trainer.hip) -------------------------------------------------------------------
@_op("rows_nan_bitmap")
def _rows_nan_bitmap(src: Tensor) -> Tensor:
    """-> int32 [ceil(rows / 32)]: the rows of src [..., D] that hold a NaN, one bit each"""
    return _ops.rows_nan_bitmap(src)


@_rows_nan_bitmap.register_fake
def _(src):
    return _i32(((src.numel() // src.shape[-1] + 31) // 32,), src)


@_op("gather_rows", mutates=("flag",))
def _gather_rows(src: Tensor, idx: Tensor, flag: Tensor) -> Tensor:
    """-> fp32 [B, D] = src[idx].float(); flag int32 [1] gets bit 0 where an index is outside the chunk"""
    return _ops.gather_rows(src, idx, flag)


@_gather_rows.register_fake
def _(src, idx, flag):
    return _f32((idx.shape[0], src.shape[-1]), src)


@_op("trainer_loss", mutates=("grads",))
def _trainer_loss(x: Tensor, recons: List[Tensor], mode: int, coef: float, grads: Tensor) -> Tensor:
    """-> losses fp32 [n]; grads fp32 [n, B, D] receives the gradient of every level's loss at its reconstruction"""
    return _ops.trainer_loss(x, recons, mode, coef, grads)[0]


@_trainer_loss.register_fake
def _(x, recons, mode, coef, grads):
    return _f32((len(recons),), x)


# ---- watch: the distributions of a list of tensors (csrc/watch.hip) ------------------------------------------------------
@_op("tensor_stats")
def _tensor_stats(tensors: List[Tensor], bins: int) -> Tensor:
    """-> int64 [T, 8 + bins]: lo, hi, mean, m2, the counts and the histogram of every tensor of the list"""
    return _ops.tensor_stats(tensors, bins)


@_tensor_stats.register_fake
def _(tensors, bins):
    device = tensors[0].device if len(tensors) else torch.device("cuda")
    return torch.empty((len(tensors), 8 + bins), dtype=torch.int64, device=device)


# ---- activity: per-unit firing counts of a model in training (csrc/activity.hip) ----------------------------------------------
@_op("activity_add_compact", mutates=("fired", "last"))
def _activity_add_compact(idx: Tensor, val: Optional[Tensor], stamp: int, fired: Tensor, last: Tensor) -> None:
    _ops.activity_add_compact(idx, val, stamp, fired, last)


@_activity_add_compact.register_fake
def _(idx, val, stamp, fired, last):
    return None


@_op("activity_add_bits", mutates=("fired", "last"))
def _activity_add_bits(zbits: Tensor, index: Optional[Tensor], stamp: int, fired: Tensor, last: Tensor) -> None:
    _ops.activity_add_bits(zbits, index, stamp, fired, last)


@_activity_add_bits.register_fake
def _(zbits, index, stamp, fired, last):
    return None


@_op("activity_add_dense", mutates=("fired", "last"))
def _activity_add_dense(latent: Tensor, stamp: int, fired: Tensor, last: Tensor) -> None:
    _ops.activity_add_dense(latent, stamp, fired, last)


@_activity_add_dense.register_fake
def _(latent, stamp, fired, last):
    return None


@_op("activity_summary", mutates=("base", "dead_out"))
def _activity_summary(fired: Tensor, base: Optional[Tensor], last: Tensor, clock: int, window: int, seg_sizes: List[int],
                      advance: bool, dead_out: Optional[Tensor]) -> Tensor:
    """-> int64 [1 + n_seg, 8 + 34]: the head words and octave bins of all units and of every segment"""
    return _ops.activity_summary(fired, base, last, clock, window, seg_sizes, advance, dead_out)


@_activity_summary.register_fake
def _(fired, base, last, clock, window, seg_sizes, advance, dead_out):
    return torch.empty((1 + len(seg_sizes), 8 + 34), dtype=torch.int64, device=fired.device)


# ---- resampling: revive dead units from high-loss rows (csrc/resample.hip) ---------------------------------------------------
@_op("resample_row_weights")
def _resample_row_weights(x: Tensor, recon: Tensor) -> Tensor:
    """-> fp64 [N]: the squared loss of every row"""
    return _ops.resample_row_weights(x, recon)


@_resample_row_weights.register_fake
def _(x, recon):
    return torch.empty((x.shape[0],), dtype=torch.float64, device=x.device)


@_op("resample_draw")
def _resample_draw(w: Tensor, u: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (rows int32 [n], report int64 [8])"""
    return _ops.resample_draw(w, u)


@_resample_draw.register_fake
def _(w, u):
    return (torch.empty((u.shape[0],), dtype=torch.int32, device=w.device),
            torch.empty((_ops.RESAMPLE_REPORT_WORDS,), dtype=torch.int64, device=w.device))


@_op("resample_alive_stats")
def _resample_alive_stats(W_enc: Tensor, logits: Optional[Tensor], dead: Tensor, n_bits: int) -> Tensor:
    """-> fp64 [2]: enc_norm_mean, logit_mean"""
    return _ops.resample_alive_stats(W_enc, logits, dead, n_bits)


@_resample_alive_stats.register_fake
def _(W_enc, logits, dead, n_bits):
    return torch.empty((2,), dtype=torch.float64, device=W_enc.device)


_RESAMPLE_WRITTEN = ("W_enc", "b_enc", "dec", "report", "m_We", "v_We", "m_be", "v_be", "m_dec", "v_dec", "last")


@_op("resample_write_table", mutates=_RESAMPLE_WRITTEN)
def _resample_write_table(W_enc: Tensor, b_enc: Tensor, dec: Tensor, dead: Tensor, rows: Tensor, x: Tensor, dec_bias: Tensor,
                          stats: Tensor, report: Tensor, m_We: Optional[Tensor], v_We: Optional[Tensor], m_be: Optional[Tensor],
                          v_be: Optional[Tensor], m_dec: Optional[Tensor], v_dec: Optional[Tensor], last: Optional[Tensor],
                          rows_seen: int, encoder_scale: float) -> None:
    _ops.resample_write_table(W_enc, b_enc, dec, dead, rows, x, dec_bias, stats, report, (m_We, v_We, m_be, v_be, m_dec, v_dec),
                              last, rows_seen, encoder_scale)


@_resample_write_table.register_fake
def _(W_enc, b_enc, dec, dead, rows, x, dec_bias, stats, report, m_We, v_We, m_be, v_be, m_dec, v_dec, last, rows_seen,
      encoder_scale):
    return None


@_op("resample_write_binary", mutates=_RESAMPLE_WRITTEN)
def _resample_write_binary(W_enc: Tensor, b_enc: Tensor, dec: Tensor, dead: Tensor, rows: Tensor, x: Tensor, dec_bias: Tensor,
                           stats: Tensor, report: Tensor, n_bits: int, m_We: Optional[Tensor], v_We: Optional[Tensor],
                           m_be: Optional[Tensor], v_be: Optional[Tensor], m_dec: Optional[Tensor], v_dec: Optional[Tensor],
                           last: Optional[Tensor], rows_seen: int, encoder_scale: float, logit_scale: Optional[float]) -> None:
    _ops.resample_write_binary(W_enc, b_enc, dec, dead, rows, x, dec_bias, stats, report, n_bits,
                               (m_We, v_We, m_be, v_be, m_dec, v_dec), last, rows_seen, encoder_scale, logit_scale)


@_resample_write_binary.register_fake
def _(W_enc, b_enc, dec, dead, rows, x, dec_bias, stats, report, n_bits, m_We, v_We, m_be, v_be, m_dec, v_dec, last, rows_seen,
      encoder_scale, logit_scale):
    return None


@_op("encode_topk_units")
def _encode_topk_units(x: Tensor, W: Tensor, bias: Optional[Tensor], units: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """-> (idx int32 [B, k] of unit ids, val fp32 [B, k]): the top-k of the listed units' pre-activations"""
    return _ops.encode_topk_units(x, W, bias, units, k)


@_encode_topk_units.register_fake
def _(x, W, bias, units, k):
    return _i32((x.shape[0], k), x), _f32((x.shape[0], k), x)


@_op("auxk_loss")
def _auxk_loss(x: Tensor, recon: Tensor, aux: Tensor, coef: float) -> Tuple[Tensor, Tensor]:
    """-> (loss fp32 0-d, grad fp32 [B, D]): the normalised auxiliary loss and its gradient at aux"""
    return _ops.auxk_loss(x, recon, aux, coef)


@_auxk_loss.register_fake
def _(x, recon, aux, coef):
    return _f32((), x), _f32(x.shape, x)


@_op("prefix_errors", mutates=("sums", "counts", "recon_out"))
def _prefix_errors(x: Tensor, idx: Tensor, val: Tensor, ks: List[int], dictionary: Tensor, n_bits: int, mult: float,
                   dec_bias: Optional[Tensor], group_rows: int, sums: Tensor, counts: Tensor,
                   recon_out: Optional[Tensor]) -> None:
    """sums [len(ks)], counts [2] += the squared error at every k' of ks from one top-K list; n_bits > 0: ``dictionary`` is the
    packed n-bit one and mult its step, n_bits == 0: an fp32 table and its scale"""
    decoder = ("packed", dictionary, n_bits, mult) if n_bits > 0 else ("table", dictionary, mult)
    _ops.prefix_errors(x, idx, val, ks, decoder, dec_bias, group_rows, sums, counts, recon_out)


@_prefix_errors.register_fake
def _(x, idx, val, ks, dictionary, n_bits, mult, dec_bias, group_rows, sums, counts, recon_out):
    return None


# ---- nested-dictionary and Multi-TopK objectives of the top-k SAEs (include/qsae_nested.h, include/qsae_multik.h) ---------
# The two families have the same five operations; an op's schema carries its argument names, so each definition below is
# written once over ``levels`` and ``grads`` and registered per family under that family's names.
def _levels_op(name: str, make, fake, levels: str, grads: str):
    fn = make(getattr(_ops, name))
    sig = inspect.signature(fn)
    renames = {"levels": levels, "grads": grads}
    fn.__signature__ = sig.replace(parameters=[p.replace(name=renames.get(n, n)) for n, p in sig.parameters.items()])
    _op(name)(fn).register_fake(fake)


def _make_decode_levels_binary(impl):
    def op(idx: Tensor, val: Tensor, packed: Tensor, D: int, n_bits: int, step: float, bias: Optional[Tensor],
           levels: List[int]) -> Tensor:
        """-> fp32 [L, B, D]: one reconstruction per level or point from the packed n-bit dictionary"""
        return impl(idx, val, packed, D, n_bits, step, bias, levels)
    return op


def _fake_decode_levels_binary(idx, val, packed, D, n_bits, step, bias, levels):
    return _f32((len(levels), idx.shape[0], D), idx)


def _make_decode_levels_table(impl):
    def op(idx: Tensor, val: Tensor, table: Tensor, scale: float, bias: Optional[Tensor], levels: List[int]) -> Tensor:
        """-> fp32 [L, B, D]: one reconstruction per level or point from an fp32 [H, D] table"""
        return impl(idx, val, table, scale, bias, levels)
    return op


def _fake_decode_levels_table(idx, val, table, scale, bias, levels):
    return _f32((len(levels), idx.shape[0], table.shape[1]), idx)


def _make_row_grad_levels(impl):
    def op(idx: Tensor, table: Tensor, step: float, grads: List[Optional[Tensor]], levels: List[int],
           g_latent: Optional[Tensor], W_enc: Optional[Tensor], want_dx: bool) -> Tuple[Tensor, Tensor, Tensor]:
        """-> (G [L, B, D], gv [B, k], dx [B, D] ([0, D] when not wanted))"""
        G, gv, dx = impl(idx, table, step, grads, levels, g_latent, W_enc, want_dx)
        return G, gv, (dx if dx is not None else _f32((0, table.shape[1]), idx))
    return op


def _fake_row_grad_levels(idx, table, step, grads, levels, g_latent, W_enc, want_dx):
    B, D = idx.shape[0], table.shape[1]
    return _f32((len(levels), B, D), idx), _f32(tuple(idx.shape), idx), _f32((B if want_dx else 0, D), idx)


def _make_unit_grad_levels(impl):
    def op(offsets: Tensor, entries: Tensor, val: Tensor, gv: Tensor, x: Tensor, G: Optional[Tensor], levels: List[int],
           logits: Tensor, n_bits: int, step: float, g_polarize: Optional[Tensor], want_encoder: bool,
           want_logits: bool) -> Tuple[Tensor, Tensor, Tensor]:
        """-> (dW_enc [H, D], db_enc [H], dlogits [H, D n_bits]); an output not wanted has 0 rows"""
        dW, db, dl = impl(offsets, entries, val, gv, x, G, levels, logits, n_bits, step, g_polarize, want_encoder, want_logits)
        D = x.shape[1]
        return (dW if dW is not None else _f32((0, D), x), db if db is not None else _f32((0,), x),
                dl if dl is not None else _f32((0, logits.shape[1]), x))
    return op


def _fake_unit_grad_levels(offsets, entries, val, gv, x, G, levels, logits, n_bits, step, g_polarize, want_encoder, want_logits):
    H, D = offsets.shape[0] - 1, x.shape[1]
    return (_f32((H if want_encoder else 0, D), x), _f32((H if want_encoder else 0,), x),
            _f32((H if want_logits else 0, logits.shape[1]), x))


def _make_table_unit_grad_levels(impl):
    def op(offsets: Tensor, entries: Tensor, val: Tensor, gv: Tensor, x: Tensor, G: Optional[Tensor], levels: List[int],
           want_encoder: bool, want_decoder: bool) -> Tuple[Tensor, Tensor, Tensor]:
        """-> (dW_enc [H, D], db_enc [H], dW_dec [D, H]); an output not wanted is empty ([0, D], [0], [D, 0])"""
        dW, db, dWd = impl(offsets, entries, val, gv, x, G, levels, want_encoder, want_decoder)
        D = x.shape[1]
        return (dW if dW is not None else _f32((0, D), x), db if db is not None else _f32((0,), x),
                dWd if dWd is not None else _f32((D, 0), x))
    return op


def _fake_table_unit_grad_levels(offsets, entries, val, gv, x, G, levels, want_encoder, want_decoder):
    H, D = offsets.shape[0] - 1, x.shape[1]
    return (_f32((H if want_encoder else 0, D), x), _f32((H if want_encoder else 0,), x),
            _f32((D, H if want_decoder else 0), x))


for _family, _levels, _grads in (("nested", "bounds", "g_levels"), ("multik", "ks", "g_points")):
    for _name, _make, _fake in (("decode_{}_binary", _make_decode_levels_binary, _fake_decode_levels_binary),
                                ("decode_{}_table", _make_decode_levels_table, _fake_decode_levels_table),
                                ("train_row_grad_{}", _make_row_grad_levels, _fake_row_grad_levels),
                                ("train_unit_grad_{}", _make_unit_grad_levels, _fake_unit_grad_levels),
                                ("train_table_unit_grad_{}", _make_table_unit_grad_levels, _fake_table_unit_grad_levels)):
        _levels_op(_name.format(_family), _make, _fake, _levels, _grads)


# ---- BatchTopK of the top-k SAEs (include/qsae_batch.h) --------------------------------------------------------------------
@_op("batch_select", mutates=("theta", "batches"))
def _batch_select(val: Tensor, n_select: int, want_val: bool, theta: Optional[Tensor], batches: Optional[Tensor],
                  lr: float) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (counts int32 [B], val_sel fp32 [B, K] ([0, K] when not wanted), report int64 [4]); theta / batches in place"""
    counts, val_sel, report = _ops.batch_select(val, n_select, want_val, theta, batches, lr)
    return counts, (val_sel if val_sel is not None else _f32((0, val.shape[1]), val)), report


@_batch_select.register_fake
def _(val, n_select, want_val, theta, batches, lr):
    B, K = val.shape
    return _i32((B,), val), _f32((B if want_val else 0, K), val), torch.empty((4,), dtype=torch.int64, device=val.device)


@_op("threshold_select")
def _threshold_select(val: Tensor, theta_dev: Optional[Tensor], theta_host: float, want_val: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (counts, val_sel, report) as batch_select; theta is theta_dev (read on the device) or, without one, theta_host"""
    counts, val_sel, report = _ops.threshold_select(val, theta_dev if theta_dev is not None else theta_host, want_val)
    return counts, (val_sel if val_sel is not None else _f32((0, val.shape[1]), val)), report


@_threshold_select.register_fake
def _(val, theta_dev, theta_host, want_val):
    B, K = val.shape
    return _i32((B,), val), _f32((B if want_val else 0, K), val), torch.empty((4,), dtype=torch.int64, device=val.device)


@_op("decode_ragged_binary")
def _decode_ragged_binary(idx: Tensor, val: Tensor, counts: Tensor, packed: Tensor, D: int, n_bits: int, step: float,
                          bias: Optional[Tensor]) -> Tensor:
    """-> fp32 [B, D]: row r decodes the first counts[r] entries of its list from the packed n-bit dictionary"""
    return _ops.decode_ragged_binary(idx, val, counts, packed, D, n_bits, step, bias)


@_decode_ragged_binary.register_fake
def _(idx, val, counts, packed, D, n_bits, step, bias):
    return _f32((idx.shape[0], D), idx)


@_op("decode_ragged_table")
def _decode_ragged_table(idx: Tensor, val: Tensor, counts: Tensor, table: Tensor, scale: float, bias: Optional[Tensor]) -> Tensor:
    """-> fp32 [B, D]: row r decodes the first counts[r] entries of its list from an fp32 [H, D] table"""
    return _ops.decode_ragged_table(idx, val, counts, table, scale, bias)


@_decode_ragged_table.register_fake
def _(idx, val, counts, table, scale, bias):
    return _f32((idx.shape[0], table.shape[1]), idx)


@_op("train_row_grad_ragged")
def _train_row_grad_ragged(idx: Tensor, counts: Tensor, table: Tensor, step: float, g_recon: Optional[Tensor],
                           g_latent: Optional[Tensor], W_enc: Optional[Tensor], want_dx: bool) -> Tuple[Tensor, Tensor]:
    """-> (gv [B, K], dx [B, D] ([0, D] when not wanted))"""
    gv, dx = _ops.train_row_grad_ragged(idx, counts, table, step, g_recon, g_latent, W_enc, want_dx)
    return gv, (dx if dx is not None else _f32((0, table.shape[1]), idx))


@_train_row_grad_ragged.register_fake
def _(idx, counts, table, step, g_recon, g_latent, W_enc, want_dx):
    return _f32(tuple(idx.shape), idx), _f32((idx.shape[0] if want_dx else 0, table.shape[1]), idx)


@_op("train_csr_ragged")
def _train_csr_ragged(idx: Tensor, counts: Tensor, H: int) -> Tuple[Tensor, Tensor]:
    """-> (offsets int32 [H + 1], entries int32 [B K])"""
    return _ops.train_csr_ragged(idx, counts, H)


@_train_csr_ragged.register_fake
def _(idx, counts, H):
    return _i32((H + 1,), idx), _i32((idx.shape[0] * idx.shape[1],), idx)


# ---- JumpReLU of the top-k SAEs (include/qsae_jump.h) ----------------------------------------------------------------------
@_op("jump_select")
def _jump_select(idx: Tensor, val: Tensor, theta: Tensor, eps: float,
                 want_band: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (idx_sel, val_sel, counts, idx_band ([0, K] when not wanted), counts_band ([0]), l0 fp32 [1], report int64 [6])"""
    idx_sel, val_sel, counts, idx_band, counts_band, l0, report = _ops.jump_select(idx, val, theta, eps, want_band)
    if not want_band:
        idx_band, counts_band = _i32((0, val.shape[1]), val), _i32((0,), val)
    return idx_sel, val_sel, counts, idx_band, counts_band, l0, report


@_jump_select.register_fake
def _(idx, val, theta, eps, want_band):
    B, K = val.shape
    return (_i32((B, K), val), _f32((B, K), val), _i32((B,), val), _i32((B if want_band else 0, K), val),
            _i32((B if want_band else 0,), val), _f32((1,), val), torch.empty((6,), dtype=torch.int64, device=val.device))


@_op("jump_threshold_grad")
def _jump_threshold_grad(offsets: Tensor, entries: Tensor, gv_band: Optional[Tensor], theta: Tensor, g_l0: Optional[Tensor],
                         B: int, K: int, eps: float) -> Tensor:
    """-> dtheta fp32 [H]"""
    return _ops.jump_threshold_grad(offsets, entries, gv_band, theta, g_l0, B, K, eps)


@_jump_threshold_grad.register_fake
def _(offsets, entries, gv_band, theta, g_l0, B, K, eps):
    return _f32((theta.shape[0],), theta)


# ---- the dense (uncapped) JumpReLU encoder (include/qsae_jump_dense.h) ------------------------------------------------------
@_op("encode_jump")
def _encode_jump(x: Tensor, W: Tensor, bias: Optional[Tensor], theta: Tensor, K: int, bandwidth: float,
                 want_band: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (idx_sel, val_sel, counts, idx_band ([0, K] when not wanted), counts_band ([0]), l0 fp32 [1], report int64 [6])"""
    idx_sel, val_sel, counts, idx_band, counts_band, l0, report = _ops.encode_jump(x, W, bias, theta, K, bandwidth, want_band)
    if not want_band:
        idx_band, counts_band = _i32((0, K), x), _i32((0,), x)
    return idx_sel, val_sel, counts, idx_band, counts_band, l0, report


@_encode_jump.register_fake
def _(x, W, bias, theta, K, bandwidth, want_band):
    B = x.shape[0]
    return (_i32((B, K), x), _f32((B, K), x), _i32((B,), x), _i32((B if want_band else 0, K), x),
            _i32((B if want_band else 0,), x), _f32((1,), x), torch.empty((6,), dtype=torch.int64, device=x.device))


# ---- the dense BatchTopK encoder (include/qsae_batch_dense.h) ----------------------------------------------------------------
@_op("encode_batch_topk", mutates=("floor_dev", "theta", "batches"))
def _encode_batch_topk(x: Tensor, W: Tensor, bias: Optional[Tensor], n_select: int, K: int, floor_dev: Optional[Tensor],
                       floor_host: float, floor_ratio: float, theta: Optional[Tensor], batches: Optional[Tensor],
                       lr: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (idx_sel int32 [B, K], val_sel fp32 [B, K], counts int32 [B], report int64 [8]); the floor is floor_dev (read and
    written on the device) or, without one, floor_host; theta / batches in place"""
    return _ops.encode_batch_topk(x, W, bias, n_select, K, floor_dev if floor_dev is not None else floor_host, floor_ratio,
                                  None if theta is None and batches is None else (theta, batches, lr))


@_encode_batch_topk.register_fake
def _(x, W, bias, n_select, K, floor_dev, floor_host, floor_ratio, theta, batches, lr):
    B = x.shape[0]
    return _i32((B, K), x), _f32((B, K), x), _i32((B,), x), torch.empty((8,), dtype=torch.int64, device=x.device)


# ---- nested levels over the ragged rows of BatchTopK (include/qsae_nested_batch.h) ------------------------------------------
@_op("decode_nested_ragged_binary")
def _decode_nested_ragged_binary(idx: Tensor, val: Tensor, counts: Tensor, packed: Tensor, D: int, n_bits: int, step: float,
                                 bias: Optional[Tensor], bounds: List[int]) -> Tuple[Tensor, Tensor]:
    """-> (levels fp32 [L, B, D], counts_below int32 [L, B]) from the first counts[r] entries of every row's list"""
    return _ops.decode_nested_ragged_binary(idx, val, counts, packed, D, n_bits, step, bias, bounds)


@_decode_nested_ragged_binary.register_fake
def _(idx, val, counts, packed, D, n_bits, step, bias, bounds):
    return _f32((len(bounds), idx.shape[0], D), idx), _i32((len(bounds), idx.shape[0]), idx)


@_op("decode_nested_ragged_table")
def _decode_nested_ragged_table(idx: Tensor, val: Tensor, counts: Tensor, table: Tensor, scale: float, bias: Optional[Tensor],
                                bounds: List[int]) -> Tuple[Tensor, Tensor]:
    """-> (levels fp32 [L, B, D], counts_below int32 [L, B]) from an fp32 [H, D] table"""
    return _ops.decode_nested_ragged_table(idx, val, counts, table, scale, bias, bounds)


@_decode_nested_ragged_table.register_fake
def _(idx, val, counts, table, scale, bias, bounds):
    return _f32((len(bounds), idx.shape[0], table.shape[1]), idx), _i32((len(bounds), idx.shape[0]), idx)


@_op("train_row_grad_nested_ragged")
def _train_row_grad_nested_ragged(idx: Tensor, counts: Tensor, table: Tensor, step: float, g_levels: List[Optional[Tensor]],
                                  bounds: List[int], g_latent: Optional[Tensor], W_enc: Optional[Tensor],
                                  want_dx: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (G [L, B, D], gv [B, K], dx [B, D] ([0, D] when not wanted))"""
    G, gv, dx = _ops.train_row_grad_nested_ragged(idx, counts, table, step, g_levels, bounds, g_latent, W_enc, want_dx)
    return G, gv, (dx if dx is not None else _f32((0, table.shape[1]), idx))


@_train_row_grad_nested_ragged.register_fake
def _(idx, counts, table, step, g_levels, bounds, g_latent, W_enc, want_dx):
    B, D = idx.shape[0], table.shape[1]
    return _f32((len(bounds), B, D), idx), _f32(tuple(idx.shape), idx), _f32((B if want_dx else 0, D), idx)


Q = torch.ops.qsae


# ---- the Python face the module classes call: ops.py's names and keyword defaults, routed through torch.ops.qsae -----------
def _none_if_empty(t: Tensor, want: bool):
    return t if want else None


def kperm_rows(src, out=None):
    return _ops.kperm_rows(src, out) if out is not None else Q.kperm_rows(src)


def encode_dense(x, W, bias, act=ACT_NONE, out=None, kperm=False):
    if out is not None or _ops.kernel_timer.enabled:                 # (out= variant and the bench's event brackets: not graph ops)
        return _ops.encode_dense(x, W, bias, act, out=out, kperm=kperm)
    return Q.encode_dense(x, W, bias, act, kperm)


def emu_pack_w(W):
    return Q.emu_pack_w(W)


def encode_dense_emu(x, Wc, meta2, bias, act=ACT_NONE):
    return Q.encode_dense_emu(x, Wc, meta2, bias, act)


def encode_bits(x, W, bias):
    return Q.encode_bits(x, W, bias)


def _bits_fp16(kind):
    def call(x, W, bias, Wq, meta):
        z, flagged = getattr(Q, f"encode_bits_{kind}")(x, W, bias, Wq, meta)
        return z, int(flagged)
    call.__name__ = call.__qualname__ = f"encode_bits_{kind}"
    return call


encode_bits_prefilter = _bits_fp16("prefilter")
encode_bits_band = _bits_fp16("band")


def topk_rows(latent, k, zero_rest):
    return Q.topk_rows(latent, k, zero_rest)


def encode_topk(x, W, bias, k, kperm=False):
    return Q.encode_topk(x, W, bias, k, kperm)


def encode_topk_latent(x, W, bias, k, kperm=False):
    return Q.encode_topk_latent(x, W, bias, k, kperm)


def prefilter_pack_w(W, bias):
    return Q.prefilter_pack_w(W, bias)


def encode_topk_prefilter(x, W, bias, Wq, meta, k, want_dense=True, dense_out=None, spec_rows=0, info=None):
    if dense_out is not None:
        return _ops.encode_topk_prefilter(x, W, bias, Wq, meta, k, want_dense, dense_out, spec_rows, info)
    idx, val, dense, flagged = Q.encode_topk_prefilter(x, W, bias, Wq, meta, k, want_dense, spec_rows)
    if info is not None:
        info["flagged_rows"] = int(flagged)
    return idx, val, _none_if_empty(dense, want_dense)


def binary_forward_prefilter(x, W, bias, Wq, meta, k, packed, n_bits, step, dec_bias, want_dense=True, spec_rows=0, info=None):
    idx, val, dense, recon, flagged = Q.binary_forward_prefilter(x, W, bias, Wq, meta, k, packed, n_bits, float(step), dec_bias,
                                                                 want_dense, spec_rows)
    if info is not None:
        info["flagged_rows"] = int(flagged)
    return idx, val, _none_if_empty(dense, want_dense), recon


def table_forward_prefilter(x, W, bias, Wq, meta, k, table, scale, dec_bias, want_dense=True, spec_rows=0, info=None):
    idx, val, dense, recon, flagged = Q.table_forward_prefilter(x, W, bias, Wq, meta, k, table, float(scale), dec_bias,
                                                                want_dense, spec_rows)
    if info is not None:
        info["flagged_rows"] = int(flagged)
    return idx, val, _none_if_empty(dense, want_dense), recon


def densify(idx, val, H, out=None):
    return _ops.densify(idx, val, H, out) if out is not None else Q.densify(idx, val, H)


def pack_binary(logits, D, n_bits, want_polarize=True, want_soft_gap=False):
    packed, pol, gap = Q.pack_binary(logits, D, n_bits)
    pol = pol if want_polarize else None
    return (packed, pol, gap) if want_soft_gap else (packed, pol)


def unpack_binary(packed, D, n_bits):
    return Q.unpack_binary(packed, D, n_bits)


def binary_soft_table(logits, D, n_bits):
    return Q.binary_soft_table(logits, D, n_bits)


def decode_binary_sparse(idx, val, packed, D, n_bits, step, bias=None):
    return Q.decode_binary_sparse(idx, val, packed, D, n_bits, float(step), bias)


def decode_table_sparse(idx, val, table, scale=1.0, bias=None):
    return Q.decode_table_sparse(idx, val, table, float(scale), bias)


def pack_ternary(w):
    return Q.pack_ternary(w)


def decode_ternary_dense(h, codes, D):
    return Q.decode_ternary_dense(h, codes, D)


def pack_matryoshka(w, wm, n_bits, abs_range, sizes=None):
    return Q.pack_matryoshka(w, wm, n_bits, float(abs_range), None if sizes is None else [int(s) for s in sizes])


def pack_matryoshka_rows(w, wm):
    return Q.pack_matryoshka_rows(w, wm)


def decode_matryoshka(zbits, H, D, n_bits, codes, scale, bias, allow_bias, sizes=None):
    return Q.decode_matryoshka(zbits, H, D, n_bits, codes, scale, bias, allow_bias, None if sizes is None else [int(s) for s in sizes],
                               False)


def decode_matryoshka_sparse(zbits, H, D, n_bits, codes_rows, scale, bias, allow_bias, sizes=None):
    return Q.decode_matryoshka(zbits, H, D, n_bits, codes_rows, scale, bias, allow_bias,
                               None if sizes is None else [int(s) for s in sizes], True)


def expand_codes_bf16(codes, D, H):
    return Q.expand_codes_bf16(codes, int(D), int(H))


def decode_ternary_dense_split(h, tq, D):
    return Q.decode_ternary_dense_split(h, tq, int(D))


def split_scale_bf16(scale):
    return Q.split_scale_bf16(scale)


def decode_matryoshka_split(zbits, H, D, n_bits, tq, s3, bias, allow_bias, sizes=None):
    return Q.decode_matryoshka_split(zbits, H, D, n_bits, tq, s3, bias, allow_bias, None if sizes is None else [int(v) for v in sizes])


def pack_bits_gt(dense, thr):
    return Q.pack_bits_gt(dense, float(thr))


def residual_update(residual, recon, scale=2.0):
    return Q.residual_update(residual, recon, float(scale))


def threshold_ge(pre, cutoff):
    return Q.threshold_ge(pre, float(cutoff))


def scale_bias_rows(acc, scale, bias):
    return Q.scale_bias_rows(acc, float(scale), bias)


def sq_err_sum(recon, x, acc=None):
    if acc is None:
        acc = torch.zeros((), dtype=torch.float64, device=x.device)
    Q.sq_err_sum(recon, x, acc)
    return acc


def activation_counts(idx, val, H, counts=None):
    if counts is None:
        counts = torch.zeros((H,), dtype=torch.int64, device=idx.device)
    Q.activation_counts(idx, val, counts)
    return counts


def activation_counts_bits(zbits, counts=None):
    if counts is None:
        counts = torch.zeros((32 * zbits.shape[1],), dtype=torch.int64, device=zbits.device)
    Q.activation_counts_bits(zbits, counts)
    return counts


def coactivation_sparse(idx, val, H, coact=None):
    if coact is None or coact.stride(0) != coact.shape[1]:
        return _ops.coactivation_sparse(idx, val, H, coact)
    Q.coactivation_sparse(idx, val, coact)
    return coact


def coactivation_bits(zbits, H, index=None, coact=None):
    if coact is None or coact.stride(0) != coact.shape[1]:
        return _ops.coactivation_bits(zbits, H, index, coact)
    Q.coactivation_bits(zbits, index, coact)
    return coact


def coactivation_partners_bits(zbits, index=None, partners=None):
    if partners is None:
        partners = torch.zeros((32 * zbits.shape[1], zbits.shape[1]), dtype=torch.int32, device=zbits.device)
    Q.coactivation_partners_bits(zbits, index, partners)
    return partners


def coactivation_partners_sparse(idx, val, H, partners=None):
    if partners is None:
        words = (int(H) + 31) // 32
        partners = torch.zeros((32 * words, words), dtype=torch.int32, device=idx.device)
    Q.coactivation_partners_sparse(idx, val, int(H), partners)
    return partners


def coactivation_partner_counts(partners, H, index=None):
    return Q.coactivation_partner_counts(partners, int(H), index)


def coactivation_partner_counts_dense(coact, row0=0):
    return Q.coactivation_partner_counts_dense(coact, int(row0))


def token_overlap_hist(asets, asize, bsets, bsize, V, k, hist=None):
    if hist is None:
        hist = torch.zeros((int(k) + 1, 2 * int(k) + 1), dtype=torch.int64, device=asets.device)
    Q.token_overlap_hist(asets, asize, bsets, bsize, int(V), int(k), hist)
    return hist


def token_lists_count(idx, val, H):
    return Q.token_lists_count(idx, val, int(H))


def token_lists_count_bits(zbits, H, index=None):
    return Q.token_lists_count_bits(zbits, index, int(H))


def token_lists_fill(workspace, offsets, row_tokens, n_entries):
    return Q.token_lists_fill(workspace, offsets, row_tokens, int(n_entries))


def token_lists_regroup(batch_offsets, segments):
    return Q.token_lists_regroup(batch_offsets, segments)


token_lists_workspace_bytes = _ops.token_lists_workspace_bytes


def top_examples_compact(idx, val, floor, base, keys):
    Q.top_examples_compact(idx, val, float(floor), int(base), keys)
    return keys


def top_examples_dense(latent, floor, base, keys):
    Q.top_examples_dense(latent, float(floor), int(base), keys)
    return keys


def top_examples_decode(keys):
    return Q.top_examples_decode(keys)


def quantization_error(logits, D, n_bits, step, margin_logit):
    return Q.quantization_error(logits, int(D), int(n_bits), float(step), float(margin_logit))


def dataset_moments_add(x, recon, group_rows, sums, counts):
    Q.dataset_moments_add(x, recon, int(group_rows), sums, counts)


TOP_EXAMPLES_MAX_N = _ops.TOP_EXAMPLES_MAX_N


def quantize_bits(x, n_bits, scale_factor, signed=True):
    return Q.quantize_bits(x, int(n_bits), float(scale_factor), bool(signed))


def cosine_compare(A, B=None, thresholds=(), bins=0, want_matrix=False):
    return Q.cosine_compare(A, B, [float(t) for t in thresholds], int(bins), bool(want_matrix))


def nearest_atoms_f32(a, b=None, k=10, exclude_self=False):
    return Q.nearest_atoms_f32(a, b, int(k), bool(exclude_self))


def kmeans_assign(atoms, centers, metric="cosine"):
    return Q.kmeans_assign(atoms, centers, str(metric))


def kmeans_update(atoms, labels, centers_old):
    return Q.kmeans_update(atoms, labels, centers_old)


def nearest_atoms_i8(a, b=None, k=10, exclude_self=False, want_duplicates=False):
    keys, dup = Q.nearest_atoms_i8(a, b, int(k), bool(exclude_self), bool(want_duplicates))
    return keys, (dup if want_duplicates else None)


def binary_soft_table_polarize(logits, D, n_bits):
    return Q.binary_soft_table_polarize(logits, int(D), int(n_bits))


def train_csr(idx, H):
    return Q.train_csr(idx, int(H))


def train_row_grad(idx, table, step, g_recon, g_latent, W_enc=None, want_dx=False):
    gv, dx = Q.train_row_grad(idx, table, float(step), g_recon, g_latent, W_enc if want_dx else None, bool(want_dx))
    return gv, (dx if want_dx else None)


def train_unit_grad(offsets, entries, val, gv, x, g_recon, logits, n_bits, step, g_polarize, want_encoder=True,
                    want_logits=True):
    dW, db, dl = Q.train_unit_grad(offsets, entries, val, gv, x, g_recon, logits, int(n_bits), float(step), g_polarize,
                                   bool(want_encoder), bool(want_logits))
    return (dW if want_encoder else None), (db if want_encoder else None), (dl if want_logits else None)


def train_col_sum(g):
    return Q.train_col_sum(g)


def train_table_unit_grad(offsets, entries, val, gv, x, g_recon, want_encoder=True, want_decoder=True):
    dW, db, dWd = Q.train_table_unit_grad(offsets, entries, val, gv, x, g_recon, bool(want_encoder), bool(want_decoder))
    return (dW if want_encoder else None), (db if want_encoder else None), (dWd if want_decoder else None)


def normalize_columns_table(W, want_table=True):
    table = Q.normalize_columns_table(W, bool(want_table))
    return table if want_table else None


# what has no tensor result (shape queries, handles of batches in flight) stays plain Python
train_supported = _ops.train_supported
normalize_columns_supported = _ops.normalize_columns_supported
encode_topk_supported = _ops.encode_topk_supported
prefilter_supported = _ops.prefilter_supported
encode_bits_prefilter_supported = _ops.encode_bits_prefilter_supported
encode_bits_band_supported = _ops.encode_bits_band_supported
decode_matryoshka_sparse_supported = _ops.decode_matryoshka_sparse_supported
split_dec_supported = _ops.split_dec_supported
encode_dense_emu_supported = _ops.encode_dense_emu_supported
matryoshka_sizes = _ops.matryoshka_sizes
binary_row_bytes = _ops.binary_row_bytes
binary_forward_prefilter_submit = _ops.binary_forward_prefilter_submit
table_forward_prefilter_submit = _ops.table_forward_prefilter_submit
encode_bits_prefilter_submit = _ops.encode_bits_prefilter_submit
release_workspaces = _ops.release_workspaces
kernel_timer = _ops.kernel_timer


# ---- model level: one node per forward() ------------------------------------------------------------------------------------
_modules = weakref.WeakValueDictionary()
_next_handle = [1]


def module_handle(module) -> int:
    """Process-local integer under which a module's forward op finds the module (its derived-weight caches, its path
    switches).  Assigned once, in the constructor (GraphForwardMixin); a traced forward reads the plain attribute."""
    h = module.__dict__.get("_qsae_handle")
    if h is None or _modules.get(h) is not module:
        h = _next_handle[0]
        _next_handle[0] += 1
        module.__dict__["_qsae_handle"] = h
        _modules[h] = module
    return h


class GraphForwardMixin:
    """For the module classes: a handle of their own, also after ``copy.deepcopy`` and unpickling (a copied ``__dict__``
    would otherwise carry the original's handle, and the copy's graph node would run the original module)."""

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k != "_qsae_handle":
                new.__dict__[k] = copy.deepcopy(v, memo)
        module_handle(new)
        return new

    def __setstate__(self, state):
        state = dict(state)
        state.pop("_qsae_handle", None)
        super().__setstate__(state)
        module_handle(self)


def _module(handle: int):
    m = _modules.get(handle)
    if m is None:
        raise RuntimeError(f"qsae: no live module behind handle {handle} (graphs that contain qsae::*_sae_forward nodes "
                           "are valid only in the process, and for the module, they were traced with)")
    return m


@_op("binary_sae_forward")
def _binary_sae_forward(x: Tensor, params: List[Tensor], handle: int, want_dense: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """BinarySAE.forward / forward_compact: -> (idx, val, dense latent ([0, H] when not wanted), reconstruction, polarize)"""
    m = _module(handle)
    idx, val, latent, recon = m._run(x, want_dense)
    # (the polarize loss is a cached per-checkpoint tensor: an op's outputs have to be fresh tensors, so it is copied)
    return idx, val, _dense_or_empty(latent, x, m.hidden_dim), recon, m.decoder.packed()["polarize"].clone()


@_binary_sae_forward.register_fake
def _(x, params, handle, want_dense):
    m = _module(handle)
    B, k = x.shape[0], m.top_k
    return (_i32((B, k), x), _f32((B, k), x), _f32((B if want_dense else 0, m.hidden_dim), x), _f32((B, m.input_dim), x),
            _f32((), x))


@_op("baseline_sae_forward")
def _baseline_sae_forward(x: Tensor, params: List[Tensor], handle: int, want_dense: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    m = _module(handle)
    idx, val, h, recon = m._run(x, want_dense)
    return idx, val, _dense_or_empty(h, x, m.encoder.linear.weight.shape[0]), recon


@_baseline_sae_forward.register_fake
def _(x, params, handle, want_dense):
    m = _module(handle)
    H, D = m.encoder.linear.weight.shape
    B, k = x.shape[0], m.topk
    return _i32((B, k), x), _f32((B, k), x), _f32((B if want_dense else 0, H), x), _f32((B, D), x)


@_op("ternary_sae_forward")
def _ternary_sae_forward(x: Tensor, params: List[Tensor], handle: int) -> Tuple[Tensor, Tensor]:
    return _module(handle)._forward_eager(x)


@_ternary_sae_forward.register_fake
def _(x, params, handle):
    m = _module(handle)
    H, D = m.encoder.linear.weight.shape
    return _f32((x.shape[0], H), x), _f32((x.shape[0], D), x)


@_op("levels_sae_forward")
def _levels_sae_forward(x: Tensor, params: List[Tensor], handle: int) -> Tuple[Tensor, Tensor]:
    """QuantizedMatryoshkaSAE / ResidualQuantizedSAE forward: -> (latent_groups [n], reconstruction_levels [n, B, D])"""
    groups, levels = _module(handle)._forward_eager(x)
    return torch.stack([g.reshape(()) for g in groups]), torch.stack(list(levels))


@_levels_sae_forward.register_fake
def _(x, params, handle):
    m = _module(handle)
    n = len(m.saes) if hasattr(m, "saes") else m.n_bits
    return _f32((n,), x), _f32((n, x.shape[0], m.input_dim), x)


# ---- QuantizedMatryoshkaSAE training: called from an autograd.Function's backward and from apply_secant_grad() only (two of
# them update a tensor in place through its pointer), never traced -- plain functions over ops.py, no dispatcher nodes ------
train_matryoshka_supported = _ops.train_matryoshka_supported
train_bits_csr_supported = _ops.train_bits_csr_supported
train_pre_bits = _ops.train_pre_bits
transpose_rows = _ops.transpose_rows
train_matryoshka_sign_rows = _ops.train_matryoshka_sign_rows
train_matryoshka_dpre = _ops.train_matryoshka_dpre
train_gemm_tn = _ops.train_gemm_tn
train_matryoshka_dsum_dense = _ops.train_matryoshka_dsum_dense
train_bits_csr = _ops.train_bits_csr
train_matryoshka_dsum_lists = _ops.train_matryoshka_dsum_lists
train_matryoshka_finish = _ops.train_matryoshka_finish
train_matryoshka_secant = _ops.train_matryoshka_secant


# ---- TernarySparseAutoencoder training: called from an autograd.Function and from the RigL mask methods only (the mask
# entry points update weight and mask in place through their pointers), never traced -- plain functions over ops.py -----------
train_ternary_supported = _ops.train_ternary_supported
train_mask_supported = _ops.train_mask_supported
train_ternary_rows = _ops.train_ternary_rows
train_ternary_dpre = _ops.train_ternary_dpre
train_ternary_dweight = _ops.train_ternary_dweight
train_mask_init = _ops.train_mask_init
train_mask_update = _ops.train_mask_update


# ---- BinaryLatentSAE training: called from an autograd.Function only (dpre updates the saved pre-activation in place through
# its pointer), never traced -- plain functions over ops.py ------------------------------------------------------------------
train_blatent_supported = _ops.train_blatent_supported
blatent_binarize = _ops.blatent_binarize
train_blatent_dpre = _ops.train_blatent_dpre
train_blatent_dweight = _ops.train_blatent_dweight


# ---- optimizer (quantizedsae_amd.optim.Adam) ------------------------------------------------------------------------------------
def adam_step(p, g, m, v, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size):
    Q.adam_step(p, g, m, v, float(one_minus_b1), float(b2), float(one_minus_b2), float(bc2_sqrt), float(eps), float(step_size))


def adam_step_prefilter(W, gW, mW, vW, bias, gb, mb, vb, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size,
                        Wq=None, meta=None):
    """-> (Wq, meta); ``Wq`` / ``meta`` given: written in place and returned"""
    if Wq is None:
        Wq = torch.empty(W.shape, dtype=torch.float16, device=W.device)
    if meta is None:
        meta = torch.empty((4,), dtype=torch.float32, device=W.device)
    Q.adam_step_prefilter(W, gW, mW, vW, bias, gb, mb, vb, float(one_minus_b1), float(b2), float(one_minus_b2),
                          float(bc2_sqrt), float(eps), float(step_size), Wq, meta)
    return Wq, meta


project_columns_supported = _ops.project_columns_supported
GRAD_NORM_HEAD = _ops.GRAD_NORM_HEAD


def project_columns(W, G):
    Q.project_columns(W, G)


def grad_norm(tensors, max_norm, coef=None, report=None):
    """-> (coef fp32 [1], report int64 [4 + T]); given: written in place and returned"""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("grad_norm: takes at least one tensor")
    if coef is None:
        coef = torch.empty((1,), dtype=torch.float32, device=tensors[0].device)
    if report is None:
        report = torch.empty((GRAD_NORM_HEAD + len(tensors),), dtype=torch.int64, device=tensors[0].device)
    Q.grad_norm(tensors, float(max_norm), coef, report)
    return coef, report


def adam_step_clipped(p, g, m, v, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size, coef=None, ema=None,
                      one_minus_decay=0.0):
    Q.adam_step_clipped(p, g, m, v, float(one_minus_b1), float(b2), float(one_minus_b2), float(bc2_sqrt), float(eps),
                        float(step_size), coef, ema, float(one_minus_decay))


def adam_step_prefilter_clipped(W, gW, mW, vW, bias, gb, mb, vb, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size,
                                coef=None, emaW=None, emab=None, one_minus_decay=0.0, Wq=None, meta=None):
    """-> (Wq, meta); ``Wq`` / ``meta`` given: written in place and returned"""
    if Wq is None:
        Wq = torch.empty(W.shape, dtype=torch.float16, device=W.device)
    if meta is None:
        meta = torch.empty((4,), dtype=torch.float32, device=W.device)
    Q.adam_step_prefilter_clipped(W, gW, mW, vW, bias, gb, mb, vb, float(one_minus_b1), float(b2), float(one_minus_b2),
                                  float(bc2_sqrt), float(eps), float(step_size), coef, emaW, emab, float(one_minus_decay),
                                  Wq, meta)
    return Wq, meta


def rows_nan_bitmap(src):
    return Q.rows_nan_bitmap(src)


def gather_rows(src, idx, flag):
    return Q.gather_rows(src, idx, flag)


def trainer_loss(x, recons, mode, coef, grads=None):
    """-> (losses fp32 [n], grads fp32 [n, B, D])"""
    recons = list(recons)
    if grads is None:
        grads = torch.empty((len(recons),) + tuple(x.shape), dtype=torch.float32, device=x.device)
    return Q.trainer_loss(x, recons, int(mode), float(coef), grads), grads


def tensor_stats(tensors, bins=64):
    """-> int64 [T, 8 + bins] on the device"""
    tensors = list(tensors)
    if not tensors:                                           # no tensor to dispatch on
        return _ops.tensor_stats(tensors, int(bins))
    return Q.tensor_stats(tensors, int(bins))


def activity_add_compact(idx, val, stamp, fired, last):
    Q.activity_add_compact(idx, val, int(stamp), fired, last)


def activity_add_bits(zbits, index, stamp, fired, last):
    Q.activity_add_bits(zbits, index, int(stamp), fired, last)


def activity_add_dense(latent, stamp, fired, last):
    Q.activity_add_dense(latent, int(stamp), fired, last)


def activity_summary(fired, base, last, clock, window, seg_sizes=(), advance=True, dead_out=None):
    """-> int64 [1 + n_seg, 8 + 34] on the device"""
    return Q.activity_summary(fired, base, last, int(clock), int(window), [int(s) for s in seg_sizes], bool(advance), dead_out)


def resample_row_weights(x, recon):
    """-> fp64 [N]"""
    return Q.resample_row_weights(x, recon)


def resample_draw(w, u):
    """-> (rows int32 [n], report int64 [8])"""
    return Q.resample_draw(w, u)


def resample_alive_stats(W_enc, logits, dead, n_bits=8):
    """-> fp64 [2]"""
    return Q.resample_alive_stats(W_enc, logits, dead, int(n_bits))


def _moments(moments):
    moments = tuple(moments) if moments is not None else (None,) * 6
    if len(moments) != 6:
        raise ValueError("moments must be (m_We, v_We, m_be, v_be, m_dec, v_dec), each a tensor or None")
    return moments


def resample_write_table(W_enc, b_enc, dec, dead, rows, x, dec_bias, stats, report, moments=None, last=None, rows_seen=0,
                         encoder_scale=0.2):
    Q.resample_write_table(W_enc, b_enc, dec, dead, rows, x, dec_bias, stats, report, *_moments(moments), last, int(rows_seen),
                           float(encoder_scale))


def resample_write_binary(W_enc, b_enc, dec, dead, rows, x, dec_bias, stats, report, n_bits, moments=None, last=None, rows_seen=0,
                          encoder_scale=0.2, logit_scale=None):
    Q.resample_write_binary(W_enc, b_enc, dec, dead, rows, x, dec_bias, stats, report, int(n_bits), *_moments(moments), last,
                            int(rows_seen), float(encoder_scale), None if logit_scale is None else float(logit_scale))


ENCODE_TOPK_UNITS_MAX_K = _ops.ENCODE_TOPK_UNITS_MAX_K


def encode_topk_units(x, W, bias, units, k):
    """-> (idx int32 [B, k], val fp32 [B, k])"""
    return Q.encode_topk_units(x, W, bias, units, int(k))


def auxk_loss(x, recon, aux, coef):
    """-> (loss fp32 0-d, grad fp32 [B, D])"""
    return Q.auxk_loss(x, recon, aux, float(coef))


def prefix_errors(x, idx, val, ks, decoder, dec_bias, group_rows, sums, counts, recon_out=None):
    """decoder = ("packed", packed, n_bits, step) or ("table", table, scale), as for the forward-in-one-call ops"""
    if decoder[0] == "packed":
        dictionary, n_bits, mult = decoder[1], int(decoder[2]), float(decoder[3])
        if n_bits < 1:
            raise ValueError(f"prefix_errors: n_bits = {n_bits} is outside 1 .. 8")
    elif decoder[0] == "table":
        dictionary, n_bits, mult = decoder[1], 0, float(decoder[2])
    else:
        raise ValueError("prefix_errors: decoder must be ('packed', packed, n_bits, step) or ('table', table, scale)")
    Q.prefix_errors(x, idx, val, [int(k) for k in ks], dictionary, n_bits, mult, dec_bias, int(group_rows), sums, counts, recon_out)


NESTED_MAX_LEVELS = _ops.NESTED_MAX_LEVELS
nested_bounds = _ops.nested_bounds


def decode_nested_binary(idx, val, packed, D, n_bits, step, bias, bounds):
    """-> fp32 [L, B, D]"""
    return Q.decode_nested_binary(idx, val, packed, int(D), int(n_bits), float(step), bias, [int(b) for b in bounds])


def decode_nested_table(idx, val, table, scale, bias, bounds):
    """-> fp32 [L, B, D]"""
    return Q.decode_nested_table(idx, val, table, float(scale), bias, [int(b) for b in bounds])


def train_row_grad_nested(idx, table, step, g_levels, bounds, g_latent, W_enc=None, want_dx=False):
    """-> (G fp32 [L, B, D], gv fp32 [B, k], dx fp32 [B, D] or None)"""
    G, gv, dx = Q.train_row_grad_nested(idx, table, float(step), list(g_levels), [int(b) for b in bounds], g_latent,
                                        W_enc if want_dx else None, bool(want_dx))
    return G, gv, (dx if want_dx else None)


def train_unit_grad_nested(offsets, entries, val, gv, x, G, bounds, logits, n_bits, step, g_polarize, want_encoder=True,
                           want_logits=True):
    dW, db, dl = Q.train_unit_grad_nested(offsets, entries, val, gv, x, G, [int(b) for b in bounds], logits, int(n_bits),
                                          float(step), g_polarize, bool(want_encoder), bool(want_logits))
    return (dW if want_encoder else None), (db if want_encoder else None), (dl if want_logits else None)


def train_table_unit_grad_nested(offsets, entries, val, gv, x, G, bounds, want_encoder=True, want_decoder=True):
    dW, db, dWd = Q.train_table_unit_grad_nested(offsets, entries, val, gv, x, G, [int(b) for b in bounds], bool(want_encoder),
                                                 bool(want_decoder))
    return (dW if want_encoder else None), (db if want_encoder else None), (dWd if want_decoder else None)


MULTIK_MAX_POINTS = _ops.MULTIK_MAX_POINTS
MULTIK_MAX_K = _ops.TRAIN_MAX_K
multik_points = _ops.multik_points


def decode_multik_binary(idx, val, packed, D, n_bits, step, bias, ks):
    """-> fp32 [P, B, D]"""
    return Q.decode_multik_binary(idx, val, packed, int(D), int(n_bits), float(step), bias, [int(k) for k in ks])


def decode_multik_table(idx, val, table, scale, bias, ks):
    """-> fp32 [P, B, D]"""
    return Q.decode_multik_table(idx, val, table, float(scale), bias, [int(k) for k in ks])


def train_row_grad_multik(idx, table, step, g_points, ks, g_latent, W_enc=None, want_dx=False):
    """-> (G fp32 [P, B, D], gv fp32 [B, K], dx fp32 [B, D] or None)"""
    G, gv, dx = Q.train_row_grad_multik(idx, table, float(step), list(g_points), [int(k) for k in ks], g_latent,
                                        W_enc if want_dx else None, bool(want_dx))
    return G, gv, (dx if want_dx else None)


def train_unit_grad_multik(offsets, entries, val, gv, x, G, ks, logits, n_bits, step, g_polarize, want_encoder=True,
                           want_logits=True):
    dW, db, dl = Q.train_unit_grad_multik(offsets, entries, val, gv, x, G, [int(k) for k in ks], logits, int(n_bits),
                                          float(step), g_polarize, bool(want_encoder), bool(want_logits))
    return (dW if want_encoder else None), (db if want_encoder else None), (dl if want_logits else None)


def train_table_unit_grad_multik(offsets, entries, val, gv, x, G, ks, want_encoder=True, want_decoder=True):
    dW, db, dWd = Q.train_table_unit_grad_multik(offsets, entries, val, gv, x, G, [int(k) for k in ks], bool(want_encoder),
                                                 bool(want_decoder))
    return (dW if want_encoder else None), (db if want_encoder else None), (dWd if want_decoder else None)


BATCH_TOPK_MAX_K = _ops.BATCH_TOPK_MAX_K


def batch_select(val, n_select, want_val=True, theta=None, batches=None, lr=0.01):
    """-> (counts int32 [B], val_sel fp32 [B, K] or None, report int64 [4])"""
    counts, val_sel, report = Q.batch_select(val, int(n_select), bool(want_val), theta, batches, float(lr))
    return counts, (val_sel if want_val else None), report


def threshold_select(val, theta, want_val=True):
    """theta: a one-element fp32 device tensor (read on the device) or a number"""
    on_dev = isinstance(theta, Tensor)
    counts, val_sel, report = Q.threshold_select(val, theta if on_dev else None, 0.0 if on_dev else float(theta), bool(want_val))
    return counts, (val_sel if want_val else None), report


def decode_ragged_binary(idx, val, counts, packed, D, n_bits, step, bias=None):
    return Q.decode_ragged_binary(idx, val, counts, packed, int(D), int(n_bits), float(step), bias)


def decode_ragged_table(idx, val, counts, table, scale=1.0, bias=None):
    return Q.decode_ragged_table(idx, val, counts, table, float(scale), bias)


def train_row_grad_ragged(idx, counts, table, step, g_recon, g_latent, W_enc=None, want_dx=False):
    """-> (gv fp32 [B, K], dx fp32 [B, D] or None)"""
    gv, dx = Q.train_row_grad_ragged(idx, counts, table, float(step), g_recon, g_latent, W_enc if want_dx else None, bool(want_dx))
    return gv, (dx if want_dx else None)


def train_csr_ragged(idx, counts, H):
    return Q.train_csr_ragged(idx, counts, int(H))


def decode_nested_ragged_binary(idx, val, counts, packed, D, n_bits, step, bias, bounds):
    """-> (levels fp32 [L, B, D], counts_below int32 [L, B])"""
    return Q.decode_nested_ragged_binary(idx, val, counts, packed, int(D), int(n_bits), float(step), bias, [int(b) for b in bounds])


def decode_nested_ragged_table(idx, val, counts, table, scale, bias, bounds):
    """-> (levels fp32 [L, B, D], counts_below int32 [L, B])"""
    return Q.decode_nested_ragged_table(idx, val, counts, table, float(scale), bias, [int(b) for b in bounds])


def train_row_grad_nested_ragged(idx, counts, table, step, g_levels, bounds, g_latent, W_enc=None, want_dx=False):
    """-> (G fp32 [L, B, D], gv fp32 [B, K], dx fp32 [B, D] or None)"""
    G, gv, dx = Q.train_row_grad_nested_ragged(idx, counts, table, float(step), list(g_levels), [int(b) for b in bounds], g_latent,
                                               W_enc if want_dx else None, bool(want_dx))
    return G, gv, (dx if want_dx else None)


JUMP_MAX_K = _ops.JUMP_MAX_K


def jump_select(idx, val, theta, eps, want_band=True):
    """-> (idx_sel, val_sel, counts, idx_band or None, counts_band or None, l0 fp32 [1], report int64 [6])"""
    idx_sel, val_sel, counts, idx_band, counts_band, l0, report = Q.jump_select(idx, val, theta, float(eps), bool(want_band))
    return idx_sel, val_sel, counts, (idx_band if want_band else None), (counts_band if want_band else None), l0, report


def jump_threshold_grad(offsets, entries, gv_band, theta, g_l0, B, K, eps):
    """-> dtheta fp32 [H]"""
    return Q.jump_threshold_grad(offsets, entries, gv_band, theta, g_l0, int(B), int(K), float(eps))


JUMP_DENSE_MAX_K = _ops.JUMP_DENSE_MAX_K


def encode_jump(x, W, bias, theta, K, bandwidth, want_band=True):
    """-> (idx_sel, val_sel, counts, idx_band or None, counts_band or None, l0 fp32 [1], report int64 [6])"""
    idx_sel, val_sel, counts, idx_band, counts_band, l0, report = Q.encode_jump(x, W, bias, theta, int(K), float(bandwidth),
                                                                                bool(want_band))
    return idx_sel, val_sel, counts, (idx_band if want_band else None), (counts_band if want_band else None), l0, report


BATCH_DENSE_MAX_K = _ops.BATCH_DENSE_MAX_K


def encode_batch_topk(x, W, bias, n_select, K, floor, floor_ratio=1.0, state=None):
    """-> (idx_sel, val_sel, counts, report int64 [8]); floor: a one-element fp32 device tensor (read and written on the device)
    or a number; state: None or (theta, batches, lr)"""
    on_dev = isinstance(floor, Tensor)
    theta, batches, lr = state if state is not None else (None, None, 0.0)
    return Q.encode_batch_topk(x, W, bias, int(n_select), int(K), floor if on_dev else None, 0.0 if on_dev else float(floor),
                               float(floor_ratio), theta, batches, float(lr))


# ---- dictionaries wider than one selection kernel: top-k over hidden slabs (include/qsae_wide.h) ----------------------------
WIDE_DEFAULT_SLAB = _ops.WIDE_DEFAULT_SLAB
wide_plan = _ops.wide_plan
encode_topk_wide_supported = _ops.encode_topk_wide_supported


@_op("merge_topk_parts", mutates=("dense",))
def _merge_topk_parts(pidx: Tensor, pval: Tensor, starts: List[int], dense: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    return _ops.merge_topk_parts(pidx, pval, starts, dense)


@_merge_topk_parts.register_fake
def _(pidx, pval, starts, dense):
    return _i32((pidx.shape[1], pidx.shape[2]), pidx), _f32((pidx.shape[1], pidx.shape[2]), pidx)


@_op("encode_topk_wide")
def _encode_topk_wide(x: Tensor, W: Tensor, bias: Optional[Tensor], k: int, Wq: Optional[Tensor], meta: Optional[Tensor],
                      want_dense: bool, slab: int, spec_rows: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    info = {}
    idx, val, dense = _ops.encode_topk_wide(x, W, bias, k, Wq=Wq, meta=meta, want_dense=want_dense, slab=slab, spec_rows=spec_rows,
                                            info=info)
    return idx, val, _dense_or_empty(dense, x, W.shape[0]), torch.tensor([info["flagged_rows"], info["slabs"]], dtype=torch.int64)


@_encode_topk_wide.register_fake
def _(x, W, bias, k, Wq, meta, want_dense, slab, spec_rows):
    B, H = x.shape[0], W.shape[0]
    return _i32((B, k), x), _f32((B, k), x), _f32((B if want_dense else 0, H), x), torch.empty((2,), dtype=torch.int64)


def merge_topk_parts(pidx, pval, starts, dense=None):
    """-> (idx int32 [B, k], val fp32 [B, k]); dense: +0 stored at the element of every entry that lost"""
    return Q.merge_topk_parts(pidx, pval, [int(h) for h in starts], dense)


def encode_topk_wide(x, W, bias, k, *, Wq=None, meta=None, want_dense=True, slab=WIDE_DEFAULT_SLAB, spec_rows=0, info=None):
    """-> (idx, val, dense latent or None); info receives flagged_rows and slabs"""
    idx, val, dense, words = Q.encode_topk_wide(x, W, bias, int(k), Wq, meta, bool(want_dense), int(slab), int(spec_rows))
    if info is not None:
        info["flagged_rows"], info["slabs"] = int(words[0]), int(words[1])
    return idx, val, _none_if_empty(dense, want_dense)
