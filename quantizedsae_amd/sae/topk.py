"""What BinarySAE and BaselineSparseAutoencoder share: both are "encoder -> top-k -> sparse decode", served by the same
three selection paths, the same forward-in-one-call / two-call entry points and the same sparse backward.  Each model keeps
what really differs: its rule for resolving ``latent_path``, its shape limits and messages, and its decoder."""
from __future__ import annotations

import torch

from .. import torch_ops as ops          # torch.ops.qsae.* (dispatcher ops over the C ABI)
from .base import PackedCache, as_f32c, require_device_input

# forward-in-one-call entry points by the kind of decoder description (see ops._decode_prefilter_args)
_FORWARD_PREFILTER = {"packed": ops.binary_forward_prefilter, "table": ops.table_forward_prefilter}
_FORWARD_PREFILTER_SUBMIT = {"packed": ops.binary_forward_prefilter_submit, "table": ops.table_forward_prefilter_submit}
#: widest top-k of forward_aux: the list width of the subset top-k kernel (qsaex_encode_topk_units)
AUX_MAX_K = ops.ENCODE_TOPK_UNITS_MAX_K


class TopKCore:
    """Mixin for a module with ``self.encoder`` (a HipEncoder without activation) and a ``_qsae_handle``: the encoder-side
    state and the top-k selection.  No parameters or buffers of its own.

    A decoder description is ``("packed", packed uint8 [H, row_bytes], n_bits, step)`` or ``("table", fp32 [H, D], scale)``."""

    def _init_topk(self) -> None:
        self._pref_cache = PackedCache()
        #: rows of the previous prefilter batch that went through the exact fallback kernels (sizes the next call's
        #: speculative fallback; per model, not per process)
        self.last_flagged_rows = 0

    def _prefilter_weights(self):
        lin = self.encoder.linear
        def build():
            Wq, meta = ops.prefilter_pack_w(lin.weight.detach(), lin.bias.detach())
            return {"Wq": Wq, "meta": meta}
        return self._pref_cache.get((lin.weight, lin.bias), build)

    def _prefilter_operands(self, x):
        """-> (x as fp32, W, b, Wq, meta): the encoder arguments of every prefilter entry point.  Taken before the
        decoder description is put together, so the fp16 copy of new weights is built before the decoder's copies."""
        lin = self.encoder.linear
        pw = self._prefilter_weights()
        return as_f32c(x), lin.weight.detach(), lin.bias.detach(), pw["Wq"], pw["meta"]

    def _spec_rows(self) -> int:
        """Flagged rows the device recomputes speculatively: only after a batch that had any."""
        return 32 if self.last_flagged_rows > 0 else 0

    def _clear_encoder_copies(self) -> None:
        """The encoder half of invalidate_packed(): the fp16 and K-interleaved copies."""
        self._pref_cache.clear()
        if hasattr(self.encoder, "_kperm_cache"):
            self.encoder._kperm_cache.clear()

    #: hidden units per slab of ``latent_path = "slabs"`` (a multiple of 256 up to 32768): the per-row top-k of every slab's row
    #: range of the encoder, through the same kernels as the other paths, merged on the device (include/qsae_wide.h).  The
    #: bits do not depend on it.
    slab_width = ops.WIDE_DEFAULT_SLAB

    def _slabs_supported(self, rows: int, K: int) -> bool:
        H, D = (int(n) for n in self.encoder.linear.weight.shape)
        return 1 <= K <= H and ops.encode_topk_wide_supported(max(rows, 1), D, H, K, int(self.slab_width))

    def _select_slabs(self, x, k: int, want_dense: bool):
        """The selection over hidden slabs: the fp16 prefilter copy (of the whole matrix: its ``meta`` bounds every row range) is
        only taken -- and, after a weight update, only rebuilt -- when some slab's shape goes through the prefilter."""
        lin = self.encoder.linear
        H, D = (int(n) for n in lin.weight.shape)
        starts = ops.wide_plan(H, k, int(self.slab_width))
        if any(ops.prefilter_supported(x.shape[0], D, h1 - h0, k) for h0, h1 in zip(starts, starts[1:])):
            xf, W, b, Wq, meta = self._prefilter_operands(x)
        else:
            xf, W, b, Wq, meta = as_f32c(x), lin.weight.detach(), lin.bias.detach(), None, None
        info = {}
        idx, val, latent = ops.encode_topk_wide(xf, W, b, k, Wq=Wq, meta=meta, want_dense=want_dense, slab=int(self.slab_width),
                                                spec_rows=self._spec_rows(), info=info)
        self.last_flagged_rows = info["flagged_rows"]
        return idx, val, latent

    def _select(self, x, k: int, path: str, want_dense: bool):
        """-> (idx, val, dense latent or None) on the resolved path; bit-identical on all four."""
        lin = self.encoder.linear
        if path == "slabs":
            return self._select_slabs(x, k, want_dense)
        if path == "prefilter":
            info = {}
            idx, val, latent = ops.encode_topk_prefilter(*self._prefilter_operands(x), k, want_dense=want_dense,
                                                         spec_rows=self._spec_rows(), info=info)
            self.last_flagged_rows = info["flagged_rows"]
            return idx, val, latent
        if path == "fused" or not want_dense:
            xp, Wp, kperm = self.encoder.operands(x)
            if want_dense:
                return ops.encode_topk_latent(xp, Wp, lin.bias, k, kperm=kperm)
            idx, val = ops.encode_topk(xp, Wp, lin.bias, k, kperm=kperm)
            return idx, val, None
        latent = self.encoder(x)                                     # inplace
        idx, val = ops.topk_rows(latent, k, zero_rest=True)          # latent * mask, in place
        return idx, val, latent

    def _select_path(self, rows: int, K: int, who: str) -> str:
        """The path ``_select`` takes for a list width K that is not the model's own top-k (the test-time k sweep, the cap of
        BatchTopK): what ``resolved_latent_path`` gives for the batch, the fused path where the prefilter does not take K."""
        H, D = (int(n) for n in self.encoder.linear.weight.shape)
        path = self.resolved_latent_path(rows)
        if path == "slabs":
            if not self._slabs_supported(rows, K):
                raise ValueError(f"{who}: the slab selection does not take input_dim = {D}, hidden_dim = {H}, k = {K} at "
                                 f"slab_width = {self.slab_width}")
            return path
        if path == "prefilter" and not ops.prefilter_supported(rows, D, H, K):
            path = "fused"
        if not ops.encode_topk_supported(max(rows, 1), D, H, K) or (path == "inplace" and H > 32768):
            raise ValueError(f"{who}: no top-k path takes input_dim = {D}, hidden_dim = {H}, k = {K} at a batch of {rows} rows")
        return path

    def _forward_prefilter(self, enc, k: int, decoder, dec_bias, want_dense: bool):
        """One call: candidate sweep, exact refinement, and every row's reconstruction as soon as the refinement kernel has
        ranked it.  ``enc`` = _prefilter_operands(x).  -> (idx, val, dense latent or None, reconstruction)"""
        info = {}
        outs = _FORWARD_PREFILTER[decoder[0]](*enc, k, *decoder[1:], dec_bias, want_dense=want_dense,
                                              spec_rows=self._spec_rows(), info=info)
        self.last_flagged_rows = info["flagged_rows"]
        return outs

    def _submit_prefilter(self, enc, k: int, decoder, dec_bias, want_dense: bool, slot: int):
        """The two-call form of _forward_prefilter: -> ops.PendingForward (nothing in here waits for the GPU)."""
        return _FORWARD_PREFILTER_SUBMIT[decoder[0]](*enc, k, *decoder[1:], dec_bias, want_dense=want_dense, slot=slot,
                                                     owner=self._qsae_handle)

    # -- AuxK: the listed (dead) units reconstruct on their own ---------------------------------------------------------
    def forward_aux(self, x, units, k_aux: int):
        """The auxiliary reconstruction ``[B, D]`` of AuxK (Gao et al. 2024), with a ``grad_fn``: every row's top-``k_aux``
        pre-activations among the units listed in ``units`` (int32, ascending, distinct, on the device -- the tracker's
        ``dead_indices``), decoded through the model's training table without the decoder bias.  The backward is
        ``sparse_backward`` on that selection: encoder weight and bias and the decoder weight (logits) of the selected units get
        a gradient; ``x``, the decoder bias and the selection get none, and there is no polarize term.  ``model.activity`` is
        not fed: an auxiliary selection is not a firing.  An empty ``units`` gives zeros without a ``grad_fn`` and launches no
        kernel of the library."""
        x = require_device_input(x, "x")
        lin = self.encoder.linear
        H, D = lin.weight.shape
        who = f"{type(self).__name__}.forward_aux"
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        if not isinstance(units, torch.Tensor) or units.dtype != torch.int32 or units.dim() != 1:
            raise ValueError(f"{who}: units must be a 1-D int32 tensor of unit ids")
        if not units.is_cuda:
            raise RuntimeError(f"units is on {units.device}: quantizedsae_amd computes on MI355X only and has no CPU fallback; "
                               "move the model and the batch to a ROCm device")
        k_aux, n = int(k_aux), units.shape[0]
        if k_aux < 1:
            raise ValueError(f"{who}: k_aux = {k_aux}; expected a number >= 1")
        if k_aux > AUX_MAX_K:
            raise ValueError(f"{who}: k_aux = {k_aux} exceeds the subset top-k kernel's limit of {AUX_MAX_K}")
        if n == 0:
            return torch.zeros((x.shape[0], D), dtype=torch.float32, device=x.device)
        if k_aux > n:
            raise ValueError(f"{who}: k_aux = {k_aux} exceeds the {n} listed units")
        if not ops.train_supported(D, k_aux):
            raise ValueError(f"{who}: the gradient kernels take input_dim a multiple of 4 up to 4096 (got {D})")
        return _AuxStep.apply(self, units, k_aux, x, lin.weight, lin.bias, self._aux_decoder()[0])


    # -- nested dictionaries (Matryoshka): one reconstruction per dictionary prefix ----------------------------------------
    @staticmethod
    def default_nested_bounds(H: int, levels: int = 4):
        """``[H >> (levels - 1), ..., H >> 1, H]``: the prefixes ``[H/8, H/4, H/2, H]`` the levels of the matryoshka classes
        are read in."""
        H, levels = int(H), int(levels)
        if not 1 <= levels <= ops.NESTED_MAX_LEVELS:
            raise ValueError(f"default_nested_bounds: levels = {levels}; 1 .. {ops.NESTED_MAX_LEVELS} are supported")
        return ops.nested_bounds([H >> (levels - 1 - l) for l in range(levels)], H, "default_nested_bounds")

    def _nested_input(self, x, bounds, who: str):
        x = require_device_input(x, "x")
        H, D = self.encoder.linear.weight.shape
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        return x, ops.nested_bounds(bounds, H, f"{type(self).__name__}.{who}")

    def forward_nested(self, x, bounds):
        """``(idx int32 [B,k], val fp32 [B,k], levels fp32 [L,B,D])`` without a ``grad_fn``: the selection of ``forward()`` and,
        for every ``bounds[l]`` (ascending, the last one ``hidden_dim``), the reconstruction from the selected units below it,
        decoded from what ``forward()`` decodes from.  All levels come from one walk over each row's list
        (csrc/nested.hip); the last level is ``forward()``'s reconstruction bit for bit."""
        with torch.no_grad():
            x, bounds = self._nested_input(x, bounds, "forward_nested")
            idx, val, _ = self._nested_select(as_f32c(x), False)
            decoder, dec_bias = self._nested_decoder()
            if decoder[0] == "packed":
                D = self.encoder.linear.weight.shape[1]
                return idx, val, ops.decode_nested_binary(idx, val, decoder[1], D, decoder[2], decoder[3], dec_bias, bounds)
            return idx, val, ops.decode_nested_table(idx, val, decoder[1], decoder[2], dec_bias, bounds)

    def _forward_train_nested(self, x, bounds, dense_latent: bool, dec_param, dec_bias):
        """-> (latent or None, tuple of L level views [B, D] of one [L, B, D] tensor, what _nested_train_decoder adds)"""
        x, bounds = self._nested_input(x, bounds, "forward_train_nested")
        lin = self.encoder.linear
        latent, levels, extra = _NestedTrainStep.apply(self, bool(dense_latent), tuple(bounds), x, lin.weight, lin.bias,
                                                       dec_param, dec_bias)
        return (latent if dense_latent else None), tuple(levels[l] for l in range(len(bounds))), extra


    # -- Multi-TopK (Gao et al. 2024): one reconstruction per rank prefix of one top-K list -------------------------------------
    @staticmethod
    def default_multi_topk(top_k: int, H: int):
        """``[top_k, min(4 * top_k, 256, H)]``: the two points of ``L(k) + L(4k) / 8``, the wider one clipped to the longest
        list of the kernels and to the dictionary; one point when the two coincide."""
        top_k, H = int(top_k), int(H)
        wide = min(4 * top_k, ops.MULTIK_MAX_K, H)
        if top_k < 1 or top_k > wide:
            raise ValueError(f"default_multi_topk: top_k = {top_k}; expected 1 .. {min(ops.MULTIK_MAX_K, H)}")
        return ops.multik_points([top_k] if wide == top_k else [top_k, wide], wide, "default_multi_topk")

    def _own_top_k(self) -> int:
        return int(self.top_k if hasattr(self, "top_k") else self.topk)

    def _multik_input(self, x, ks, who: str):
        x = require_device_input(x, "x")
        H, D = self.encoder.linear.weight.shape
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        who = f"{type(self).__name__}.{who}"
        try:
            K = int(list(ks)[-1])
        except (TypeError, IndexError, ValueError):
            raise ValueError(f"{who}: ks must be a non-empty sequence of ints, got {ks!r}") from None
        if K > H:
            raise ValueError(f"{who}: ks = {list(ks)} ends above hidden_dim = {H}")
        return x, ops.multik_points(ks, K, who), who

    def forward_multi_topk(self, x, ks):
        """``(latent fp32 [B,H], recons fp32 [P,B,D])`` without a ``grad_fn``: ONE selection at ``K = ks[-1]`` through the
        model's own selection paths, and for every ``ks[p]`` (ascending) the reconstruction from the entries ranked below it,
        decoded from what ``forward()`` decodes from -- bit for bit the model rebuilt with ``top_k = ks[p]``.  The latent is the
        whole list's.  Every dictionary row is gathered once for up to four points (csrc/multi_topk.hip)."""
        with torch.no_grad():
            x, ks, who = self._multik_input(x, ks, "forward_multi_topk")
            xf = as_f32c(x)
            idx, val, latent = self._select(xf, ks[-1], self._select_path(xf.shape[0], ks[-1], who), True)
            decoder, dec_bias = self._nested_decoder()
            if decoder[0] == "packed":
                D = self.encoder.linear.weight.shape[1]
                return latent, ops.decode_multik_binary(idx, val, decoder[1], D, decoder[2], decoder[3], dec_bias, ks)
            return latent, ops.decode_multik_table(idx, val, decoder[1], decoder[2], dec_bias, ks)

    def forward_train_multi_topk(self, x, ks, *, dense_latent: bool = True):
        """The tuple of the model's ``forward_train_nested`` with a ``grad_fn`` -- ``(latent [B,H] or None, (recon_0, ...,
        recon_{P-1}))``, ``BinarySAE`` adds its polarize term -- where ``recon_p`` [B,D] decodes, through the model's training
        table, the ``ks[p]`` best-ranked entries of ONE top-``ks[-1]`` list per row; the points are the rows of one [P,B,D]
        tensor and the latent is the whole list's.  ``training.multi_topk_loss`` consumes it.  The backward is one sparse pass:
        ``train_row_grad_multik`` -> ``train_csr`` -> the model's rank-keyed unit-gradient op -> ``train_col_sum(G[0])``.
        ``model.activity`` is fed once, with the ranks below the model's own top-k only.  With ``ks = [top_k]`` outputs and
        gradients are ``forward_train``'s bit for bit."""
        x, ks, who = self._multik_input(x, ks, "forward_train_multi_topk")
        lin = self.encoder.linear
        D = lin.weight.shape[1]
        if not ops.train_supported(D, ks[-1]):
            raise ValueError(f"{who}: the gradient kernels take input_dim a multiple of 4 up to 4096 (got {D})")
        if x.shape[0] * ks[-1] >= 2 ** 31:
            raise ValueError(f"{who}: batch * K = {x.shape[0] * ks[-1]} is not below 2^31")
        latent, points, extra = _MultiTopKTrainStep.apply(self, bool(dense_latent), tuple(ks), x, lin.weight, lin.bias,
                                                          self.decoder.weight, self.decoder.bias)
        out = ((latent if dense_latent else None), tuple(points[p] for p in range(len(ks))))
        return out if extra is None else out + (extra,)

    # -- BatchTopK: the B k largest pre-activations of the batch, ragged rows ------------------------------------------------
    def _batch_topk_input(self, x, who: str):
        x = require_device_input(x, "x")
        H, D = self.encoder.linear.weight.shape
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        return x, f"{type(self).__name__}.{who}"

    def _select_cap(self, xf, cap: int, who: str):
        """-> (idx, val) [B, cap]: one selection at the list width ``cap`` through the model's own paths, no dense latent"""
        idx, val, _ = self._select(xf, cap, self._select_path(xf.shape[0], cap, who), False)
        return idx, val

    def _decode_ragged(self, idx, val, counts, decoder, dec_bias):
        if decoder[0] == "packed":
            D = self.encoder.linear.weight.shape[1]
            return ops.decode_ragged_binary(idx, val, counts, decoder[1], D, decoder[2], decoder[3], dec_bias)
        return ops.decode_ragged_table(idx, val, counts, decoder[1], decoder[2], dec_bias)

    def forward_batch_topk(self, x, ctl):
        """``(idx int32 [B,K], val_sel fp32 [B,K], counts int32 [B], reconstruction [B,D])`` without a ``grad_fn``: the
        ``B * ctl.k`` largest pre-activations of the whole batch (no ReLU in front, as in ``forward()``), selected from every
        row's top-``K`` list with K = ``ctl.cap`` (``training.BatchTopK``).  Row r keeps the first ``counts[r]`` entries of
        its list; ``val_sel`` is the list's values with +0 behind them, so ``(idx, val_sel)`` reads like any compact
        selection.  Decoded from what ``forward()`` decodes from, ``counts[r]`` entries per row.  ``ctl.counts`` and
        ``ctl.report`` are left on the device; the threshold state is not moved (``forward_train_batch_topk`` does that)."""
        with torch.no_grad():
            x, who = self._batch_topk_input(x, "forward_batch_topk")
            xf = as_f32c(x)
            idx, val = self._select_cap(xf, ctl.cap, who)
            counts, val_sel, report = ops.batch_select(val, xf.shape[0] * ctl.k)
            ctl.record(counts, report)
            decoder, dec_bias = self._nested_decoder()
            return idx, val_sel, counts, self._decode_ragged(idx, val_sel, counts, decoder, dec_bias)

    def forward_threshold(self, x, ctl_or_theta, cap=None):
        """Evaluation with the global threshold BatchTopK learned: ``(idx, val_sel, counts, reconstruction)`` as
        ``forward_batch_topk``, where row r keeps every entry of its top-``cap`` list that is ``>=`` the threshold.
        ``ctl_or_theta``: a ``training.BatchTopK`` (its threshold is read on the device, ``cap`` defaults to its cap) or a
        number (``cap`` defaults to ``min(256, hidden_dim)``)."""
        with torch.no_grad():
            x, who = self._batch_topk_input(x, "forward_threshold")
            idx, val_sel, counts, report = self._select_threshold(as_f32c(x), ctl_or_theta, cap, who)
            if hasattr(ctl_or_theta, "record"):
                ctl_or_theta.record(counts, report)
            decoder, dec_bias = self._nested_decoder()
            return idx, val_sel, counts, self._decode_ragged(idx, val_sel, counts, decoder, dec_bias)

    def _select_threshold(self, xf, ctl_or_theta, cap, who: str):
        """-> (idx, val_sel, counts, report): every entry of the rows' top-``cap`` lists that is >= the threshold"""
        H = int(self.encoder.linear.weight.shape[0])
        if hasattr(ctl_or_theta, "theta") and hasattr(ctl_or_theta, "cap"):
            theta = ctl_or_theta.state(xf.device)[0]
            cap = ctl_or_theta.cap if cap is None else int(cap)
        else:
            theta, cap = float(ctl_or_theta), (min(ops.BATCH_TOPK_MAX_K, H) if cap is None else int(cap))
        if not 1 <= cap <= min(ops.BATCH_TOPK_MAX_K, H):
            raise ValueError(f"{who}: cap = {cap}; expected 1 .. {min(ops.BATCH_TOPK_MAX_K, H)}")
        idx, val = self._select_cap(xf, cap, who)
        counts, val_sel, report = ops.threshold_select(val, theta)
        return idx, val_sel, counts, report

    def forward_train_batch_topk(self, x, ctl, *, dense_latent: bool = True):
        """The tuple of the model's ``forward_train`` with a ``grad_fn``, under the batch-wide selection of
        ``forward_batch_topk``: the latent holds ``B * ctl.k`` entries in all, ``counts[r]`` of them in row r, and the
        reconstruction decodes those through the model's training table.  Moves ``ctl``'s threshold state (on the device, in the
        selection's kernel chain) and feeds ``model.activity`` with the selected entries only.  The backward walks the ragged
        rows: ``train_row_grad_ragged`` -> ``train_csr_ragged`` -> the model's unit-gradient op -> ``train_col_sum``;
        ``BinarySAE`` keeps its polarize term.  With ``ctl.cap == ctl.k`` every entry is selected and outputs and gradients
        are ``forward_train``'s bit for bit."""
        x, who = self._batch_topk_input(x, "forward_train_batch_topk")
        lin = self.encoder.linear
        D = lin.weight.shape[1]
        if not ops.train_supported(D, ctl.cap):
            raise ValueError(f"{who}: the gradient kernels take input_dim a multiple of 4 up to 4096 (got {D})")
        if x.shape[0] * ctl.cap >= 2 ** 31:
            raise ValueError(f"{who}: batch * cap = {x.shape[0] * ctl.cap} is not below 2^31")
        dec_param, dec_bias = self.decoder.weight, self.decoder.bias
        latent, recon, extra = _BatchTopKTrainStep.apply(self, ctl, bool(dense_latent), x, lin.weight, lin.bias, dec_param,
                                                         dec_bias)
        out = ((latent if dense_latent else None), recon)
        return out if extra is None else out + (extra,)


    # -- Matryoshka BatchTopK: nested levels over the ragged rows ------------------------------------------------------------
    def _decode_nested_ragged(self, idx, val, counts, decoder, dec_bias, bounds):
        """-> (levels [L, B, D], counts_below [L, B])"""
        if decoder[0] == "packed":
            D = self.encoder.linear.weight.shape[1]
            return ops.decode_nested_ragged_binary(idx, val, counts, decoder[1], D, decoder[2], decoder[3], dec_bias, bounds)
        return ops.decode_nested_ragged_table(idx, val, counts, decoder[1], decoder[2], dec_bias, bounds)

    def forward_nested_batch_topk(self, x, ctl, bounds):
        """``(idx int32 [B,K], val_sel fp32 [B,K], counts int32 [B], levels fp32 [L,B,D])`` without a ``grad_fn``: the selection
        of ``forward_batch_topk`` and, for every ``bounds[l]`` (ascending, the last one ``hidden_dim``), the reconstruction from
        the selected units below it, decoded from what ``forward()`` decodes from.  All levels come from one walk over the first
        ``counts[r]`` entries of each row's list (csrc/nested_ragged.hip); an entry behind the prefix is never read; the last
        level is ``forward_batch_topk``'s reconstruction.  ``ctl.counts`` and ``ctl.report`` are recorded as there, and
        ``ctl.level_counts`` (int32 [L,B], on the device) holds every row's selected entries below each bound."""
        with torch.no_grad():
            x, who = self._batch_topk_input(x, "forward_nested_batch_topk")
            bounds = ops.nested_bounds(bounds, self.encoder.linear.weight.shape[0], who)
            xf = as_f32c(x)
            idx, val = self._select_cap(xf, ctl.cap, who)
            counts, val_sel, report = ops.batch_select(val, xf.shape[0] * ctl.k)
            ctl.record(counts, report)
            decoder, dec_bias = self._nested_decoder()
            levels, ctl.level_counts = self._decode_nested_ragged(idx, val_sel, counts, decoder, dec_bias, bounds)
            return idx, val_sel, counts, levels

    def forward_nested_threshold(self, x, ctl_or_theta, bounds, cap=None):
        """``forward_nested_batch_topk`` with the selection of ``forward_threshold``: row r keeps every entry of its top-``cap``
        list that is ``>=`` the threshold (``ctl_or_theta``: a ``training.BatchTopK`` or a number, as there).  With a
        ``BatchTopK``, ``counts``, ``report`` and ``level_counts`` are recorded on it."""
        return self._nested_threshold(x, ctl_or_theta, bounds, cap)[:4]

    def _nested_threshold(self, x, ctl_or_theta, bounds, cap):
        """-> (idx, val_sel, counts, levels, counts_below [L, B]) of forward_nested_threshold"""
        with torch.no_grad():
            x, who = self._batch_topk_input(x, "forward_nested_threshold")
            bounds = ops.nested_bounds(bounds, self.encoder.linear.weight.shape[0], who)
            idx, val_sel, counts, report = self._select_threshold(as_f32c(x), ctl_or_theta, cap, who)
            decoder, dec_bias = self._nested_decoder()
            levels, below = self._decode_nested_ragged(idx, val_sel, counts, decoder, dec_bias, bounds)
            if hasattr(ctl_or_theta, "record"):
                ctl_or_theta.record(counts, report)
                ctl_or_theta.level_counts = below
            return idx, val_sel, counts, levels, below

    def forward_train_nested_batch_topk(self, x, ctl, bounds, *, dense_latent: bool = True):
        """The tuple of the model's ``forward_train_nested`` with a ``grad_fn`` -- ``training.nested_loss`` consumes it
        unchanged -- under the batch-wide selection of ``forward_batch_topk``: the training recipe of the Matryoshka SAEs of
        Bussmann et al.  ``recon_l`` decodes, through the model's training table, the selected units below ``bounds[l]`` from
        the first ``counts[r]`` entries of every row.  Moves ``ctl``'s threshold state (on the device, in the selection's
        kernel chain), records ``ctl.counts``, ``ctl.report`` and ``ctl.level_counts``, and feeds ``model.activity`` once, with
        the selected entries only.  The backward walks the ragged rows: ``train_row_grad_nested_ragged`` ->
        ``train_csr_ragged`` -> the model's nested unit-gradient op -> ``train_col_sum(G[0])``.  With ``ctl.cap == ctl.k`` it
        is ``forward_train_nested`` bit for bit, with ``bounds = [hidden_dim]`` ``forward_train_batch_topk``."""
        x, who = self._batch_topk_input(x, "forward_train_nested_batch_topk")
        lin = self.encoder.linear
        H, D = lin.weight.shape
        bounds = ops.nested_bounds(bounds, H, who)
        if not ops.train_supported(D, ctl.cap):
            raise ValueError(f"{who}: the gradient kernels take input_dim a multiple of 4 up to 4096 (got {D})")
        if x.shape[0] * ctl.cap >= 2 ** 31:
            raise ValueError(f"{who}: batch * cap = {x.shape[0] * ctl.cap} is not below 2^31")
        latent, levels, extra = _NestedBatchTopKTrainStep.apply(self, ctl, bool(dense_latent), tuple(bounds), x, lin.weight,
                                                                lin.bias, self.decoder.weight, self.decoder.bias)
        out = ((latent if dense_latent else None), tuple(levels[l] for l in range(len(bounds))))
        return out if extra is None else out + (extra,)


    # -- dense BatchTopK: the batch-wide selection over the pre-activations above a floor, no top-K sweep in between -----------
    def _batch_topk_dense_input(self, x, ctl, who: str):
        x, who = self._batch_topk_input(x, who)
        if not getattr(ctl, "dense", False):
            raise ValueError(f"{who}: the controller was not made with dense=True (training.BatchTopK(model, dense=True))")
        return x, who

    def _select_batch_dense(self, xf, ctl, W_enc, b_enc, who: str, train: bool):
        """-> (idx, val_sel, counts) of the batch-wide selection through ``ops.encode_batch_topk`` (csrc/batch_dense.hip): the
        bits of ``_select_cap`` + ``ops.batch_select`` within every row's prefix, for any floor.  ``train``: moves the threshold
        state and the floor word; a controller whose floor was never seeded runs the capped selection once and seeds the floor
        from its report, on the device.  Without ``train`` neither is moved, and an unseeded controller selects capped."""
        n_select = xf.shape[0] * ctl.k
        state = ctl.state(xf.device) + (ctl.threshold_lr,) if train else None
        if not ctl.floor_seeded:
            idx, val = self._select_cap(xf, ctl.cap, who)
            theta, batches, lr = state if train else (None, None, 0.01)
            counts, val_sel, report = ops.batch_select(val, n_select, True, theta, batches, lr)
            if train:
                ctl.seed_floor(report)
            ctl.record(counts, report)
            return idx, val_sel, counts
        floor = ctl.floor_state(xf.device)
        idx, val_sel, counts, report = ops.encode_batch_topk(xf, as_f32c(W_enc.detach()), None if b_enc is None else b_enc.detach(),
                                                             n_select, ctl.cap, floor if train else floor.clone(), ctl.floor_ratio,
                                                             state)
        ctl.record(counts, report)
        return idx, val_sel, counts

    def forward_batch_topk_dense(self, x, ctl):
        """The tuple of ``forward_batch_topk`` from the dense encoder (``ops.encode_batch_topk``, csrc/batch_dense.hip): the same
        counts, the same values and the same units within every row's prefix, bit for bit, whatever the floor of ``ctl`` (a
        ``training.BatchTopK(model, dense=True)``); ``idx`` holds -1 behind the first ``counts[r]`` places.  Neither the
        threshold state nor the floor is moved.  ``ctl.report_dense`` holds the dense encoder's eight words."""
        with torch.no_grad():
            x, who = self._batch_topk_dense_input(x, ctl, "forward_batch_topk_dense")
            lin = self.encoder.linear
            idx, val_sel, counts = self._select_batch_dense(as_f32c(x), ctl, lin.weight, lin.bias, who, False)
            decoder, dec_bias = self._nested_decoder()
            return idx, val_sel, counts, self._decode_ragged(idx, val_sel, counts, decoder, dec_bias)

    def forward_train_batch_topk_dense(self, x, ctl, *, dense_latent: bool = True):
        """``forward_train_batch_topk`` with the selection of ``forward_batch_topk_dense``: the same tuple, the same backward
        over the ragged rows, the same bits.  Moves ``ctl``'s threshold state and its floor on the device."""
        x, who = self._batch_topk_dense_input(x, ctl, "forward_train_batch_topk_dense")
        lin = self.encoder.linear
        D = lin.weight.shape[1]
        if not ops.train_supported(D, ctl.cap):
            raise ValueError(f"{who}: the gradient kernels take input_dim a multiple of 4 up to 4096 (got {D})")
        if x.shape[0] * ctl.cap >= 2 ** 31:
            raise ValueError(f"{who}: batch * cap = {x.shape[0] * ctl.cap} is not below 2^31")
        latent, recon, extra = _BatchTopKDenseTrainStep.apply(self, ctl, bool(dense_latent), x, lin.weight, lin.bias,
                                                              self.decoder.weight, self.decoder.bias)
        out = ((latent if dense_latent else None), recon)
        return out if extra is None else out + (extra,)

    def forward_nested_batch_topk_dense(self, x, ctl, bounds):
        """The tuple of ``forward_nested_batch_topk`` with the selection of ``forward_batch_topk_dense``."""
        with torch.no_grad():
            x, who = self._batch_topk_dense_input(x, ctl, "forward_nested_batch_topk_dense")
            bounds = ops.nested_bounds(bounds, self.encoder.linear.weight.shape[0], who)
            lin = self.encoder.linear
            idx, val_sel, counts = self._select_batch_dense(as_f32c(x), ctl, lin.weight, lin.bias, who, False)
            decoder, dec_bias = self._nested_decoder()
            levels, ctl.level_counts = self._decode_nested_ragged(idx, val_sel, counts, decoder, dec_bias, bounds)
            return idx, val_sel, counts, levels

    def forward_train_nested_batch_topk_dense(self, x, ctl, bounds, *, dense_latent: bool = True):
        """``forward_train_nested_batch_topk`` with the selection of ``forward_batch_topk_dense``: the same tuple, the same
        backward, the same bits."""
        x, who = self._batch_topk_dense_input(x, ctl, "forward_train_nested_batch_topk_dense")
        lin = self.encoder.linear
        H, D = lin.weight.shape
        bounds = ops.nested_bounds(bounds, H, who)
        if not ops.train_supported(D, ctl.cap):
            raise ValueError(f"{who}: the gradient kernels take input_dim a multiple of 4 up to 4096 (got {D})")
        if x.shape[0] * ctl.cap >= 2 ** 31:
            raise ValueError(f"{who}: batch * cap = {x.shape[0] * ctl.cap} is not below 2^31")
        latent, levels, extra = _NestedBatchTopKDenseTrainStep.apply(self, ctl, bool(dense_latent), tuple(bounds), x, lin.weight,
                                                                     lin.bias, self.decoder.weight, self.decoder.bias)
        out = ((latent if dense_latent else None), tuple(levels[l] for l in range(len(bounds))))
        return out if extra is None else out + (extra,)


    # -- JumpReLU: one learned threshold per unit, a subset of every row's list --------------------------------------------
    def _jumprelu_input(self, x, jr, who: str):
        x, who = self._batch_topk_input(x, who)
        H = int(self.encoder.linear.weight.shape[0])
        if not hasattr(jr, "log_threshold") or tuple(jr.log_threshold.shape) != (H,):
            raise ValueError(f"{who}: expected a training.JumpReLU over hidden_dim = {H} units")
        if not 1 <= jr.cap <= min(ops.JUMP_MAX_K, H):
            raise ValueError(f"{who}: cap = {jr.cap}; expected 1 .. {min(ops.JUMP_MAX_K, H)}")
        return x, who

    def forward_jumprelu(self, x, jr):
        """``(idx_sel int32 [B,K], val_sel fp32 [B,K], counts int32 [B], reconstruction [B,D])`` without a ``grad_fn``: of every
        row's top-``K`` list (K = ``jr.cap``, ``training.JumpReLU``; no ReLU in front, as in ``forward()``) the entries above
        their unit's threshold ``exp(jr.log_threshold)``, moved to the front of the row in list order; ``val_sel`` is +0 behind
        the first ``counts[r]`` places, so ``(idx_sel, val_sel)`` reads like any compact selection.  Decoded from what
        ``forward()`` decodes from, ``counts[r]`` entries per row.  ``jr.counts`` and ``jr.report`` are left on the device."""
        with torch.no_grad():
            x, who = self._jumprelu_input(x, jr, "forward_jumprelu")
            xf = as_f32c(x)
            idx, val = self._select_cap(xf, jr.cap, who)
            idx_sel, val_sel, counts, _, _, _, report = ops.jump_select(idx, val, jr.thresholds(), jr.bandwidth, want_band=False)
            jr.record(counts, report)
            decoder, dec_bias = self._nested_decoder()
            return idx_sel, val_sel, counts, self._decode_ragged(idx_sel, val_sel, counts, decoder, dec_bias)

    def forward_train_jumprelu(self, x, jr, *, dense_latent: bool = True):
        """The tuple of the model's ``forward_train`` with a ``grad_fn`` and ``l0`` -- the mean number of firing units per row, a
        0-dim tensor -- appended as its last element, under the selection of ``forward_jumprelu``.  The reconstruction decodes
        the selected entries through the model's training table.  Feeds ``model.activity`` with the selected entries only.  The
        backward is ``sparse_backward`` over the compacted ragged rows, unchanged: a selected entry passes its gradient straight
        through.  Only when ``jr.log_threshold`` needs a gradient it goes on over the entries within half a bandwidth of their
        threshold, selected or not: ``train_row_grad_ragged`` (no dx) -> ``train_csr_ragged`` -> ``jump_threshold_grad``, the
        rectangle-kernel pseudo-derivative of the JumpReLU and of the Heaviside step in ``l0``; torch's ``exp`` backward turns it
        into the gradient of the log-parameter."""
        x, who = self._jumprelu_input(x, jr, "forward_train_jumprelu")
        lin = self.encoder.linear
        D = lin.weight.shape[1]
        if not ops.train_supported(D, jr.cap):
            raise ValueError(f"{who}: the gradient kernels take input_dim a multiple of 4 up to 4096 (got {D})")
        if x.shape[0] * jr.cap >= 2 ** 31:
            raise ValueError(f"{who}: batch * cap = {x.shape[0] * jr.cap} is not below 2^31")
        latent, recon, extra, l0 = _JumpReLUTrainStep.apply(self, jr, bool(dense_latent), x, lin.weight, lin.bias,
                                                            self.decoder.weight, self.decoder.bias, jr.log_threshold.exp())
        out = ((latent if dense_latent else None), recon)
        return (out if extra is None else out + (extra,)) + (l0,)

    # -- dense JumpReLU: the thresholds in the encoder's epilogue, no top-K list in between ----------------------------------
    def forward_jumprelu_dense(self, x, jr):
        """The tuple of ``forward_jumprelu`` from the dense encoder (``ops.encode_jump``, csrc/jump_dense.hip): every unit of a
        row whose pre-activation exceeds its threshold, found among all ``hidden_dim`` pre-activations -- no top-``cap`` list,
        no certificate.  ``idx_sel`` holds the firing units by value descending, then unit ascending, the first K = ``jr.cap``
        of them when more fire, and -1 (``val_sel``: +0) behind the first ``counts[r]`` places.  ``jr.report`` holds the dense
        encoder's six words (``jr.report_names``): a truncated row is one with more than K firing units."""
        with torch.no_grad():
            x, who = self._jumprelu_input(x, jr, "forward_jumprelu_dense")
            lin = self.encoder.linear
            idx_sel, val_sel, counts, _, _, _, report = ops.encode_jump(as_f32c(x), as_f32c(lin.weight.detach()), lin.bias,
                                                                        jr.thresholds(), jr.cap, jr.bandwidth, want_band=False)
            jr.record(counts, report, dense=True)
            decoder, dec_bias = self._nested_decoder()
            return idx_sel, val_sel, counts, self._decode_ragged(idx_sel, val_sel, counts, decoder, dec_bias)

    def forward_train_jumprelu_dense(self, x, jr, *, dense_latent: bool = True):
        """``forward_train_jumprelu`` with the selection of ``forward_jumprelu_dense``: the same tuple, the same backward over
        the ragged rows.  ``l0`` counts every firing unit, also those of a truncated row beyond its K-th."""
        x, who = self._jumprelu_input(x, jr, "forward_train_jumprelu_dense")
        lin = self.encoder.linear
        D = lin.weight.shape[1]
        if not ops.train_supported(D, jr.cap):
            raise ValueError(f"{who}: the gradient kernels take input_dim a multiple of 4 up to 4096 (got {D})")
        if x.shape[0] * jr.cap >= 2 ** 31:
            raise ValueError(f"{who}: batch * cap = {x.shape[0] * jr.cap} is not below 2^31")
        latent, recon, extra, l0 = _JumpReLUDenseTrainStep.apply(self, jr, bool(dense_latent), x, lin.weight, lin.bias,
                                                                 self.decoder.weight, self.decoder.bias, jr.log_threshold.exp())
        out = ((latent if dense_latent else None), recon)
        return (out if extra is None else out + (extra,)) + (l0,)


class _JumpReLUTrainStep(torch.autograd.Function):
    """forward_train_jumprelu and its gradient: _BatchTopKTrainStep with ``jump_select`` in place of ``batch_select`` -- the
    lists are the compacted [B, K] ones, of which row r uses the first counts[r] entries -- and ``theta`` as one more
    differentiable input (include/qsae_jump.h)."""

    @staticmethod
    def _select(model, jr, xf, W_enc, b_enc, th, want_band):
        """-> (idx_sel, val_sel, counts, idx_band, counts_band, l0); records the report on ``jr``"""
        idx, val = model._select_cap(xf, jr.cap, f"{type(model).__name__}.forward_train_jumprelu")
        idx_sel, val_sel, counts, idx_band, counts_band, l0, report = ops.jump_select(idx, val, th, jr.bandwidth, want_band=want_band)
        jr.record(counts, report)
        return idx_sel, val_sel, counts, idx_band, counts_band, l0

    @staticmethod
    def forward(ctx, model, jr, dense_latent, x, W_enc, b_enc, dec_param, b_dec, theta):
        return _JumpReLUTrainStep._run(ctx, _JumpReLUTrainStep._select, model, jr, dense_latent, x, W_enc, b_enc, b_dec, theta)

    @staticmethod
    def _run(ctx, select, model, jr, dense_latent, x, W_enc, b_enc, b_dec, theta):
        table, step, extra = model._nested_train_decoder()
        xf = as_f32c(x.detach())
        th = as_f32c(theta.detach())
        idx_sel, val_sel, counts, idx_band, counts_band, l0 = select(model, jr, xf, W_enc, b_enc, th, ctx.needs_input_grad[8])
        recon = ops.decode_ragged_table(idx_sel, val_sel, counts, table, step, b_dec.detach())
        latent = ops.densify(idx_sel, val_sel, table.shape[0]) if dense_latent else None
        if model.activity is not None:
            model.activity.add_compact(idx_sel, val_sel)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx_sel, val_sel, counts, table, th, idx_band, counts_band)
        ctx.model, ctx.step, ctx.x_dtype, ctx.eps = model, step, x.dtype, jr.bandwidth
        return latent, recon, extra, l0.reshape(())

    @staticmethod
    def backward(ctx, g_latent, g_recon, g_extra, g_l0):
        xf, idx_sel, val_sel, counts, table, th, idx_band, counts_band = ctx.saved_tensors
        model, needs = ctx.model, ctx.needs_input_grad[3:8]

        def unit_grad(offsets, entries, gv):
            return model._batch_unit_grad(offsets, entries, val_sel, gv, xf, g_recon, g_extra, needs[1] or needs[2], needs[3])
        grads = sparse_backward(idx_sel, table, ctx.step, g_recon, g_latent, model.encoder.linear.weight, model.decoder.bias,
                                needs, ctx.x_dtype, unit_grad, counts=counts)
        dtheta = None
        if ctx.needs_input_grad[8] and idx_band is not None:
            B, K = idx_band.shape
            gv_band = None
            if g_recon is not None or g_latent is not None:
                gv_band, _ = ops.train_row_grad_ragged(idx_band, counts_band, table, ctx.step, g_recon, g_latent, None, False)
            offsets, entries = ops.train_csr_ragged(idx_band, counts_band, table.shape[0])
            dtheta = ops.jump_threshold_grad(offsets, entries, gv_band, th, None if g_l0 is None else g_l0.reshape(1), B, K,
                                             ctx.eps)
        return (None,) * 3 + grads + (dtheta,)


class _JumpReLUDenseTrainStep(_JumpReLUTrainStep):
    """forward_train_jumprelu_dense and its gradient: _JumpReLUTrainStep with ``encode_jump`` in place of ``_select_cap`` +
    ``jump_select`` (include/qsae_jump_dense.h).  Everything behind the selection takes the lists unchanged: every reader goes by
    ``counts``, or drops the -1 behind a row's prefix (``densify``, ``activity.add_compact``)."""

    @staticmethod
    def _select(model, jr, xf, W_enc, b_enc, th, want_band):
        idx_sel, val_sel, counts, idx_band, counts_band, l0, report = ops.encode_jump(
            xf, as_f32c(W_enc.detach()), None if b_enc is None else b_enc.detach(), th, jr.cap, jr.bandwidth, want_band=want_band)
        jr.record(counts, report, dense=True)
        return idx_sel, val_sel, counts, idx_band, counts_band, l0

    @staticmethod
    def forward(ctx, model, jr, dense_latent, x, W_enc, b_enc, dec_param, b_dec, theta):
        return _JumpReLUTrainStep._run(ctx, _JumpReLUDenseTrainStep._select, model, jr, dense_latent, x, W_enc, b_enc, b_dec, theta)


class _NestedBatchTopKTrainStep(torch.autograd.Function):
    """forward_train_nested_batch_topk and its gradient: _BatchTopKTrainStep's selection and ragged lists ([B, K] with stride K,
    row r uses the first counts[r] entries), _NestedTrainStep's levels (the rows of ONE output tensor, whose gradient's suffix
    sums G reach the dictionary rows; include/qsae_nested_batch.h).  The model supplies what those two ask for."""

    @staticmethod
    def forward(ctx, model, ctl, dense_latent, bounds, x, W_enc, b_enc, dec_param, b_dec):
        table, step, extra = model._nested_train_decoder()
        xf = as_f32c(x.detach())
        idx, val = model._select_cap(xf, ctl.cap, f"{type(model).__name__}.forward_train_nested_batch_topk")
        theta, batches = ctl.state(xf.device)
        counts, val_sel, report = ops.batch_select(val, xf.shape[0] * ctl.k, True, theta, batches, ctl.threshold_lr)
        ctl.record(counts, report)
        levels, ctl.level_counts = ops.decode_nested_ragged_table(idx, val_sel, counts, table, step, b_dec.detach(), bounds)
        latent = ops.densify(idx, val_sel, table.shape[0]) if dense_latent else None
        if model.activity is not None:
            model.activity.add_compact(idx, val_sel)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val_sel, counts, table)
        ctx.model, ctx.step, ctx.bounds, ctx.x_dtype = model, step, bounds, x.dtype
        return latent, levels, extra

    @staticmethod
    def backward(ctx, g_latent, g_levels, g_extra):
        xf, idx, val_sel, counts, table = ctx.saved_tensors
        model, bounds, needs = ctx.model, ctx.bounds, ctx.needs_input_grad[4:9]

        def unit_grad(offsets, entries, gv, G):
            return model._levels_unit_grad("nested", offsets, entries, val_sel, gv, xf, G, bounds, g_extra, needs[1] or needs[2],
                                           needs[3])
        return (None,) * 4 + levels_backward((idx, counts), table, ctx.step, bounds, g_latent, g_levels, g_extra,
                                             model.encoder.linear.weight, needs, ctx.x_dtype,
                                             ops.train_row_grad_nested_ragged, ops.train_csr_ragged, unit_grad)


class _BatchTopKTrainStep(torch.autograd.Function):
    """forward_train_batch_topk and its gradient.  The model supplies ``_nested_train_decoder() -> (table [H, D], step, extra
    output or None)`` and ``_batch_unit_grad(offsets, entries, val, gv, x, g_recon, g_extra, want_encoder, want_decoder)``, its
    unit-gradient kernel; the lists are [B, K] with stride K, of which row r uses the first counts[r] entries."""

    @staticmethod
    def forward(ctx, model, ctl, dense_latent, x, W_enc, b_enc, dec_param, b_dec):
        table, step, extra = model._nested_train_decoder()
        xf = as_f32c(x.detach())
        idx, val = model._select_cap(xf, ctl.cap, f"{type(model).__name__}.forward_train_batch_topk")
        theta, batches = ctl.state(xf.device)
        counts, val_sel, report = ops.batch_select(val, xf.shape[0] * ctl.k, True, theta, batches, ctl.threshold_lr)
        ctl.record(counts, report)
        recon = ops.decode_ragged_table(idx, val_sel, counts, table, step, b_dec.detach())
        latent = ops.densify(idx, val_sel, table.shape[0]) if dense_latent else None
        if model.activity is not None:
            model.activity.add_compact(idx, val_sel)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val_sel, counts, table)
        ctx.model, ctx.step, ctx.x_dtype = model, step, x.dtype
        return latent, recon, extra

    @staticmethod
    def backward(ctx, g_latent, g_recon, g_extra):
        xf, idx, val_sel, counts, table = ctx.saved_tensors
        model, needs = ctx.model, ctx.needs_input_grad[3:8]

        def unit_grad(offsets, entries, gv):
            return model._batch_unit_grad(offsets, entries, val_sel, gv, xf, g_recon, g_extra, needs[1] or needs[2], needs[3])
        return (None,) * 3 + sparse_backward(idx, table, ctx.step, g_recon, g_latent, model.encoder.linear.weight,
                                             model.decoder.bias, needs, ctx.x_dtype, unit_grad, counts=counts)


class _BatchTopKDenseTrainStep(_BatchTopKTrainStep):
    """forward_train_batch_topk_dense and its gradient: _BatchTopKTrainStep with ``encode_batch_topk`` in place of ``_select_cap``
    + ``batch_select`` (include/qsae_batch_dense.h).  Everything behind the selection takes the lists unchanged: every reader goes
    by ``counts``, or drops the -1 behind a row's prefix (``densify``, ``activity.add_compact``)."""

    @staticmethod
    def forward(ctx, model, ctl, dense_latent, x, W_enc, b_enc, dec_param, b_dec):
        table, step, extra = model._nested_train_decoder()
        xf = as_f32c(x.detach())
        idx, val_sel, counts = model._select_batch_dense(xf, ctl, W_enc, b_enc,
                                                         f"{type(model).__name__}.forward_train_batch_topk_dense", True)
        recon = ops.decode_ragged_table(idx, val_sel, counts, table, step, b_dec.detach())
        latent = ops.densify(idx, val_sel, table.shape[0]) if dense_latent else None
        if model.activity is not None:
            model.activity.add_compact(idx, val_sel)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val_sel, counts, table)
        ctx.model, ctx.step, ctx.x_dtype = model, step, x.dtype
        return latent, recon, extra


class _NestedBatchTopKDenseTrainStep(_NestedBatchTopKTrainStep):
    """forward_train_nested_batch_topk_dense and its gradient: _NestedBatchTopKTrainStep with the selection of
    _BatchTopKDenseTrainStep."""

    @staticmethod
    def forward(ctx, model, ctl, dense_latent, bounds, x, W_enc, b_enc, dec_param, b_dec):
        table, step, extra = model._nested_train_decoder()
        xf = as_f32c(x.detach())
        idx, val_sel, counts = model._select_batch_dense(xf, ctl, W_enc, b_enc,
                                                         f"{type(model).__name__}.forward_train_nested_batch_topk_dense", True)
        levels, ctl.level_counts = ops.decode_nested_ragged_table(idx, val_sel, counts, table, step, b_dec.detach(), bounds)
        latent = ops.densify(idx, val_sel, table.shape[0]) if dense_latent else None
        if model.activity is not None:
            model.activity.add_compact(idx, val_sel)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val_sel, counts, table)
        ctx.model, ctx.step, ctx.bounds, ctx.x_dtype = model, step, bounds, x.dtype
        return latent, levels, extra


class _MultiTopKTrainStep(torch.autograd.Function):
    """forward_train_multi_topk and its gradient.  The model supplies ``_nested_train_decoder() -> (table [H, D], step, extra
    output or None)`` and ``_levels_unit_grad("multik", offsets, entries, val, gv, x, G, ks, g_extra, want_encoder, want_decoder)``.  The
    points are the rows of ONE output tensor, so a loss over them sends one gradient [P, B, D] back; its suffix sums
    G[p] = g[p] + G[p + 1] are what reaches the dictionary row of an entry whose rank first appears in point p
    (include/qsae_multik.h)."""

    @staticmethod
    def forward(ctx, model, dense_latent, ks, x, W_enc, b_enc, dec_param, b_dec):
        table, step, extra = model._nested_train_decoder()
        xf = as_f32c(x.detach())
        who = f"{type(model).__name__}.forward_train_multi_topk"
        idx, val, latent = model._select(xf, ks[-1], model._select_path(xf.shape[0], ks[-1], who), dense_latent)
        points = ops.decode_multik_table(idx, val, table, step, b_dec.detach(), ks)
        if model.activity is not None:
            own = min(model._own_top_k(), ks[-1])             # a rank behind the model's own top-k is not a firing
            if own == ks[-1]:
                model.activity.add_compact(idx, val)
            elif own > 0:
                model.activity.add_compact(idx[:, :own].contiguous(), val[:, :own].contiguous())
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val, table)
        ctx.model, ctx.step, ctx.ks, ctx.x_dtype = model, step, ks, x.dtype
        return latent, points, extra

    @staticmethod
    def backward(ctx, g_latent, g_points, g_extra):
        xf, idx, val, table = ctx.saved_tensors
        model, ks, needs = ctx.model, ctx.ks, ctx.needs_input_grad[3:8]

        def unit_grad(offsets, entries, gv, G):
            return model._levels_unit_grad("multik", offsets, entries, val, gv, xf, G, ks, g_extra, needs[1] or needs[2], needs[3])
        return (None,) * 3 + levels_backward((idx,), table, ctx.step, ks, g_latent, g_points, g_extra, model.encoder.linear.weight,
                                             needs, ctx.x_dtype, ops.train_row_grad_multik, ops.train_csr, unit_grad)


class _NestedTrainStep(torch.autograd.Function):
    """forward_train_nested and its gradient.  The model supplies ``_nested_train_decoder() -> (table [H, D], step, extra
    output or None)``, ``_nested_select(x, want_dense) -> (idx, val, latent)`` and ``_levels_unit_grad("nested", offsets, entries,
    val, gv, x, G, bounds, g_extra, want_encoder, want_decoder)``.  The levels are the rows of ONE output tensor, so a loss over them
    sends one gradient [L, B, D] back; its suffix sums G[l] = g[l] + G[l + 1] are what reaches the dictionary rows of level l
    (include/qsae_nested.h)."""

    @staticmethod
    def forward(ctx, model, dense_latent, bounds, x, W_enc, b_enc, dec_param, b_dec):
        table, step, extra = model._nested_train_decoder()
        xf = as_f32c(x.detach())
        idx, val, latent = model._nested_select(xf, dense_latent)
        levels = ops.decode_nested_table(idx, val, table, step, b_dec.detach(), bounds)
        if model.activity is not None:
            model.activity.add_compact(idx, val)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val, table)
        ctx.model, ctx.step, ctx.bounds, ctx.x_dtype = model, step, bounds, x.dtype
        return latent, levels, extra

    @staticmethod
    def backward(ctx, g_latent, g_levels, g_extra):
        xf, idx, val, table = ctx.saved_tensors
        model, bounds, needs = ctx.model, ctx.bounds, ctx.needs_input_grad[3:8]

        def unit_grad(offsets, entries, gv, G):
            return model._levels_unit_grad("nested", offsets, entries, val, gv, xf, G, bounds, g_extra, needs[1] or needs[2],
                                           needs[3])
        return (None,) * 3 + levels_backward((idx,), table, ctx.step, bounds, g_latent, g_levels, g_extra,
                                             model.encoder.linear.weight, needs, ctx.x_dtype, ops.train_row_grad_nested,
                                             ops.train_csr, unit_grad)


class _AuxStep(torch.autograd.Function):
    """forward_aux and its gradient.  The model supplies ``_aux_decoder() -> (decoder parameter, table [H, D], step)`` and
    ``_aux_unit_grad(offsets, entries, val, gv, x, g_recon, want_encoder, want_decoder)``, its unit-gradient kernel without
    a polarize term."""

    @staticmethod
    def forward(ctx, model, units, k_aux, x, W_enc, b_enc, dec_param):
        _, table, step = model._aux_decoder()
        xf = as_f32c(x.detach())
        idx, val = ops.encode_topk_units(xf, W_enc.detach(), b_enc.detach(), units, k_aux)
        recon = ops.decode_table_sparse(idx, val, table, step, None)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val, table)
        ctx.model, ctx.step, ctx.x_dtype = model, step, x.dtype
        return recon

    @staticmethod
    def backward(ctx, g_recon):
        xf, idx, val, table = ctx.saved_tensors
        model = ctx.model
        need_W, need_b, need_dec = ctx.needs_input_grad[4:7]
        if g_recon is None or not (need_W or need_b or need_dec):
            return (None,) * 7

        def unit_grad(offsets, entries, gv):
            return model._aux_unit_grad(offsets, entries, val, gv, xf, g_recon, need_W or need_b, need_dec)
        grads = sparse_backward(idx, table, ctx.step, g_recon, None, model.encoder.linear.weight, None,
                                (False, need_W, need_b, need_dec, False), ctx.x_dtype, unit_grad)
        return (None, None, None) + grads[:4]


class SubmittedForward:
    """What ``forward_submit`` returns: ``pending`` (a batch in flight) or ``outs`` (computed eagerly) as
    (idx, val, latent, reconstruction); ``to_result`` is the model's function from those four to its return tuple."""

    def __init__(self, model, pending, outs, to_result):
        self._model, self._pending, self._outs, self._to_result = model, pending, outs, to_result

    def result(self):
        with torch.no_grad():
            if self._pending is not None:
                self._outs = self._pending.finish()
                self._model.last_flagged_rows = self._pending.flagged_rows
                self._pending = None
            return self._to_result(*self._outs)


def sparse_backward(idx, table, step: float, g_recon, g_latent, W_enc, dec_bias, needs, x_dtype, unit_grad, counts=None):
    """The gradient of encoder -> top-k -> ``step * table`` rows + bias, from the k selected entries of each row:
    gv = g_latent[r, h] + step <g_recon[r], table[h]> and dx per row, then ``unit_grad(offsets, entries, gv) ->
    (dW_enc, db_enc, d_decoder)`` per unit over the rows that selected it (the one step that differs between the models),
    and the decoder bias' column sum.  ``needs`` = (need_x, need_W, need_b, need_decoder, need_dec_bias).  ``counts``: the
    ragged rows of BatchTopK, row r using the first counts[r] entries of its list.
    -> (dx, dW_enc, db_enc, d_decoder, db_dec), None where not needed."""
    need_x, need_W, need_b, need_dec, need_bd = needs
    lists = (idx,) if counts is None else (idx, counts)
    row_grad, csr = (ops.train_row_grad, ops.train_csr) if counts is None else (ops.train_row_grad_ragged, ops.train_csr_ragged)
    want_units = need_W or need_b or need_dec
    dx = dW = db = ddec = dbd = None
    if need_x or want_units:
        gv, dx = row_grad(*lists, table, step, g_recon, g_latent, W_enc.detach(), want_dx=need_x)
        if want_units:
            offsets, entries = csr(*lists, table.shape[0])
            dW, db, ddec = unit_grad(offsets, entries, gv)
    if need_bd:
        dbd = ops.train_col_sum(g_recon) if g_recon is not None else torch.zeros_like(dec_bias)
    if dx is not None and dx.dtype != x_dtype:
        dx = dx.to(x_dtype)
    return (dx if need_x else None, dW if need_W else None, db if need_b else None, ddec if need_dec else None, dbd)


def levels_backward(lists, table, step: float, levels, g_latent, g_levels, g_extra, W_enc, needs, x_dtype, row_grad, csr,
                    unit_grad):
    """``sparse_backward`` for an objective with one reconstruction per level or point (the rows of ONE output tensor, whose
    gradient ``g_levels`` is [L, B, D] or None): ``row_grad`` (``ops.train_row_grad_nested`` / ``_multik`` /
    ``_nested_ragged``) turns it into the suffix sums G, gv and dx over ``lists`` -- ``(idx,)`` or ``(idx, counts)`` --,
    ``csr`` groups the lists by unit, ``unit_grad(offsets, entries, gv, G) -> (dW_enc, db_enc, d_decoder)`` is the model's,
    and every level adds the bias, so its gradient is the whole sum G[0].  Nothing is computed when no gradient came in.
    -> (dx, dW_enc, db_enc, d_decoder, db_dec), None where not needed."""
    need_x, need_W, need_b, need_dec, need_bd = needs
    want_units = need_W or need_b or need_dec
    dx = dW = db = ddec = dbd = None
    if (need_x or want_units or need_bd) and not (g_latent is None and g_levels is None and g_extra is None):
        g_list = [None] * len(levels) if g_levels is None else [g_levels[l] for l in range(len(levels))]
        G, gv, dx = row_grad(*lists, table, step, g_list, levels, g_latent, W_enc.detach(), want_dx=need_x)
        if want_units:
            offsets, entries = csr(*lists, table.shape[0])
            dW, db, ddec = unit_grad(offsets, entries, gv, G)
        if need_bd:
            dbd = ops.train_col_sum(G[0])
        if dx is not None and dx.dtype != x_dtype:
            dx = dx.to(x_dtype)
    return (dx if need_x else None, dW if need_W else None, db if need_b else None, ddec if need_dec else None,
            dbd if need_bd else None)
