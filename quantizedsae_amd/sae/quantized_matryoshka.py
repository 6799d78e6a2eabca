"""QuantizedMatryoshkaSAE: sigmoid encoder binarised at 0.5, nested {-2,0,+2} dictionaries with
per-row scales (reference: sae/quantized_matryoshka.py:10-220)."""
from __future__ import annotations

from typing import List, Tuple

import torch
import torch.nn as nn

from .. import torch_ops as ops          # torch.ops.qsae.* (dispatcher ops over the C ABI)
from .base import HipEncoder, PackedCache, SparseAutoencoder, as_f32c, dense_encoder_backward, require_device_input

def nested_sizes(in_features: int, n_bits: int) -> List[int]:
    """Level sizes [1,1,2,4,...] scaled to in_features, remainder in the last level
    (sae/quantized_matryoshka.py:25-38)."""
    sizes = [1 if i < 2 else 2 ** (i - 1) for i in range(n_bits)]
    total = sum(sizes)
    if total != in_features:
        f = in_features / total
        sizes = [max(1, int(s * f)) for s in sizes]
        sizes[-1] = in_features - sum(sizes[:-1])
    return sizes


def _pad32(n: int) -> int:
    return (n + 31) // 32 * 32


class QuantizedMatryoshkaDecoder(nn.Module):
    """``forward(latent [B,H]) -> (latent_group: list of n 0-d tensors, result: list of n [B,D])``.

    Level i covers a slice of the hidden units; S = sgn(sigmoid(w) >= .5) + sgn(sigmoid(wm) >= .5),
    scale_j = 2^(n-i-2) * quant_step / (||S_j|| + 1e-8), z = latent > 0.5,
    recon_i = recon_{i-1} + (scale * z) @ S (+ bias once, after level 0).

    The packed form keeps S/2 as 2-bit fields (hidden index contiguous) and fp32 scales; the kernels
    need every level boundary on a multiple of 32, so odd level sizes are padded with inert units
    (S = 0, z = 0) at pack time.
    """

    def __init__(self, in_features, out_features, abs_range=4, n_bits=8, top_k=None, joint_gradient=False,
                 allow_bias=True):
        super().__init__()
        self._ctx = [None] * n_bits
        self.joint_gradient = joint_gradient
        self.in_features = in_features
        self.out_features = out_features
        self.n_bits = n_bits
        self.abs_range = abs_range
        self.quant_step = abs_range / (2 ** (n_bits - 1))
        self.top_k = top_k
        self.allow_bias = allow_bias
        self.nested_dictionary_size = nested_sizes(in_features, n_bits)
        self.weight = nn.Parameter(torch.empty(in_features, out_features))
        self.weight_mirror = nn.Parameter(torch.empty(in_features, out_features))
        self.bias = nn.Parameter(torch.zeros(out_features))
        nn.init.xavier_uniform_(self.weight)
        nn.init.xavier_uniform_(self.weight_mirror)
        self._cache = PackedCache()
        self._train_cache = PackedCache()
        self._train_ctx = None           # what apply_secant_grad() needs of the last forward_train (the reference's _ctx)

    # -- layout ---------------------------------------------------------------------------------
    @property
    def padded_sizes(self) -> List[int]:
        return [_pad32(s) for s in self.nested_dictionary_size]

    @property
    def needs_padding(self) -> bool:
        return self.padded_sizes != list(self.nested_dictionary_size)

    def padded_index(self, device) -> torch.Tensor:
        """For every padded hidden slot the source hidden unit, or -1 for an inert pad slot."""
        out = []
        start = 0
        for s, p in zip(self.nested_dictionary_size, self.padded_sizes):
            out.append(torch.arange(start, start + s, device=device))
            if p > s:
                out.append(torch.full((p - s,), -1, device=device, dtype=torch.long))
            start += s
        return torch.cat(out)

    def packed(self) -> dict:
        def build():
            w = require_device_input(self.weight.detach(), "decoder.weight")
            wm = self.weight_mirror.detach()
            sizes = list(self.nested_dictionary_size)
            st = {"sizes": sizes, "H": self.in_features, "index": None}
            if self.needs_padding:
                index = self.padded_index(w.device)
                valid = index >= 0
                Hp = int(index.numel())
                wp = torch.ones((Hp, self.out_features), device=w.device)
                wmp = -torch.ones((Hp, self.out_features), device=w.device)   # S = 0 on pad rows
                wp[valid] = w[index[valid]]
                wmp[valid] = wm[index[valid]]
                w, wm = wp, wmp
                st.update(sizes=self.padded_sizes, H=Hp, index=index)
            codes, scale = ops.pack_matryoshka(w, wm, self.n_bits, self.abs_range, st["sizes"])
            st.update(codes=codes, scale=scale)
            if ops.decode_matryoshka_sparse_supported(self.out_features):
                st["codes_rows"] = ops.pack_matryoshka_rows(w, wm)      # hidden-major copy for the sparse walk
            ends = [sum(st["sizes"][:i + 1]) for i in range(self.n_bits)]
            if ops.split_dec_supported(1, st["H"], self.out_features) and all(e % 64 == 0 for e in ends):
                st["tq"] = ops.expand_codes_bf16(codes, self.out_features, st["H"])      # bf16 image for the split kernel
                st["s3"] = ops.split_scale_bf16(scale)                                    # three bf16 terms of 2 scale
            return st
        return self._cache.get((self.weight, self.weight_mirror), build)

    # -- decode ---------------------------------------------------------------------------------
    #: "auto" | "fp32": the dense decoder on the bf16 matrix pipe where the kernel covers the shape (out_features 512,
    #: padded hidden size and level boundaries % 64 == 0), or always the exact-fp32 MFMA chain.  See STEWeights.precision.
    precision = "auto"
    #: the sparse walk beats the dense contraction below ~12 % active units (measured: 15 ms at 16 %, 23 ms dense)
    SPARSE_MAX_ACTIVE_FRACTION = 0.12

    #: rows of a batch whose active units decide between the decoders: evenly spaced, so the choice is a function of the
    #: batch alone, and few, so the count costs one small kernel (the count over every row of a 65536-row batch takes 0.6 ms
    #: at 0.6 % density and 2 ms at 50 %: per-unit atomics)
    DENSITY_SAMPLE_ROWS = 64

    def active_fraction(self, zbits: torch.Tensor) -> float:
        """Fraction of active units over DENSITY_SAMPLE_ROWS evenly spaced rows of this batch of z bits (rows
        floor(i B / n), i < n; every row of a batch of at most n rows): one popcount kernel and one host read."""
        B, n = zbits.shape[0], self.DENSITY_SAMPLE_ROWS
        if B == 0:
            return 0.0
        rows = zbits if B <= n else zbits.index_select(0, torch.arange(n, device=zbits.device) * B // n)
        return float(ops.activation_counts_bits(rows).sum().item()) / (rows.shape[0] * 32 * zbits.shape[1])

    def decode_bits(self, zbits: torch.Tensor, sparse=None) -> Tuple[list, list]:
        """zbits: int32-packed [B, H_padded/32] in the packed (padded) hidden order.  ``sparse``: walk the active
        units only (same outputs as the exact-fp32 chain); None = decide from this batch's own activation density.  The sparse
        walk and the bf16 split decoder round their sums in different orders, so the choice is a function of the z bits and
        the attributes alone -- never of earlier batches or of how far the GPU has got."""
        B = zbits.shape[0]
        if sparse is None:
            sparse = self.sparse_walk_possible(B) and self.active_fraction(zbits) < self.SPARSE_MAX_ACTIVE_FRACTION
        levels, counts = self._decode_levels(zbits, sparse)
        groups = (counts.to(torch.float64) / max(B, 1)).to(torch.float32)
        return [groups[i] for i in range(self.n_bits)], [levels[i] for i in range(self.n_bits)]

    def sparse_walk_possible(self, rows: int) -> bool:
        """Whether decode_bits looks at the activation density of a batch of ``rows`` rows at all."""
        return "codes_rows" in self.packed() and rows > 0 and self.SPARSE_MAX_ACTIVE_FRACTION > 0

    def _decode_levels(self, zbits: torch.Tensor, sparse: bool):
        """-> (levels fp32 [n_bits, B, D], active-unit counts int64 [n_bits]) on the decoder ``sparse`` selects."""
        st = self.packed()
        B = zbits.shape[0]
        if sparse and "codes_rows" in st:
            levels, counts = ops.decode_matryoshka_sparse(zbits, st["H"], self.out_features, self.n_bits,
                                                          st["codes_rows"], st["scale"], self.bias.detach(),
                                                          self.allow_bias, st["sizes"])
        elif self.precision != "fp32" and "tq" in st and B * zbits.stride(0) * 4 < (1 << 32):
            # dense activations: z_j * 2 scale_j as three exact bf16 terms against the {-1, 0, +1} dictionary on the bf16
            # matrix pipe (fp32 accumulation; qsae_decode_matryoshka_split)
            levels, counts = ops.decode_matryoshka_split(zbits, st["H"], self.out_features, self.n_bits, st["tq"], st["s3"],
                                                         self.bias.detach(), self.allow_bias, st["sizes"])
        else:
            levels, counts = ops.decode_matryoshka(zbits, st["H"], self.out_features, self.n_bits, st["codes"],
                                                   st["scale"], self.bias.detach(), self.allow_bias, st["sizes"])
        return levels, counts

    def forward(self, latent):
        with torch.no_grad():
            latent = require_device_input(latent, "latent")
            if latent.dtype != torch.float32:
                latent = latent.float()
            st = self.packed()
            if st["index"] is not None:
                index = st["index"]
                padded = torch.zeros((latent.shape[0], st["H"]), device=latent.device)
                padded[:, index >= 0] = latent[:, index[index >= 0]]
                latent = padded
            return self.decode_bits(ops.pack_bits_gt(latent, 0.5))

    # -- training -------------------------------------------------------------------------------
    def train_pack(self) -> dict:
        """What the backward needs besides packed(): the fp32 image S [H_padded, D] of the dictionary in the packed hidden
        order (the K-contiguous operand of the dz contraction) and the int32 slot -> unit map of a padded model."""
        def build():
            st = self.packed()
            index = st["index"].to(torch.int32) if st["index"] is not None else None
            return {"S": ops.train_matryoshka_sign_rows(self.weight.detach(), self.weight_mirror.detach(), index),
                    "index": index}
        return self._train_cache.get((self.weight, self.weight_mirror), build)

    def apply_secant_grad(self):
        """The secant correction of the reference's training loop (sae/quantized_matryoshka.py:145-190, joint_gradient=False):
        ``weight.grad[h, d] -= c cnt_h scale_h^2 Bs[h, d] sw (1 - sw)`` and the same for the mirror, in place, in one HIP
        pass, with cnt / scale / B of the last ``forward_train`` (c = 1 / (B D))."""
        tc = self._train_ctx
        if tc is None:
            raise RuntimeError("apply_secant_grad() needs the context of a forward_train(); forward() leaves none")
        if self.weight.grad is None or self.weight_mirror.grad is None:
            raise RuntimeError("apply_secant_grad() needs decoder.weight.grad and decoder.weight_mirror.grad (run backward first)")
        if (self.weight._version, self.weight_mirror._version) != tc["versions"]:
            raise RuntimeError("decoder.weight / weight_mirror changed since the last forward_train(): its signs and scales "
                               "no longer describe them")
        with torch.no_grad():
            counts = ops.activation_counts_bits(tc["zbits"])
            ops.train_matryoshka_secant(self.weight.grad, self.weight_mirror.grad, counts,
                                        1.0 / tc["rows"] / self.out_features, tc["scale"], tc["index"],
                                        self.weight.detach(), self.weight_mirror.detach())


class QuantizedMatryoshkaSAE(ops.GraphForwardMixin, SparseAutoencoder):
    """``forward(x) -> (latent_groups, reconstruction_levels)``; ``top_k`` is stored and unused, as
    in the reference (sae/quantized_matryoshka.py:192-220)."""

    def __init__(self, input_dim, hidden_dim, top_k, abs_range=4, n_bits=8, allow_bias=True):
        super().__init__(input_dim, hidden_dim)
        self.n_bits = n_bits
        self.abs_range = abs_range
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.allow_bias = allow_bias
        self.top_k = top_k
        lin = nn.Linear(input_dim, hidden_dim)
        nn.init.xavier_uniform_(lin.weight, gain=1)
        nn.init.zeros_(lin.bias)
        self.encoder = HipEncoder(lin, nn.Sigmoid())
        self.decoder = QuantizedMatryoshkaDecoder(hidden_dim, input_dim, abs_range=abs_range, n_bits=n_bits,
                                                  top_k=self.top_k, allow_bias=self.allow_bias)
        self._enc_cache = PackedCache()
        ops.module_handle(self)

    def _encoder_params(self):
        """Encoder weight/bias in the decoder's packed hidden order (inert pad units get a zero row
        and bias -1, so their z bit is 0)."""
        lin = self.encoder.linear
        if not self.decoder.needs_padding:
            return lin.weight.detach(), lin.bias.detach()

        def build():
            index = self.decoder.padded_index(lin.weight.device)
            valid = index >= 0
            W = torch.zeros((index.numel(), self.input_dim), device=lin.weight.device)
            b = -torch.ones((index.numel(),), device=lin.weight.device)
            W[valid] = lin.weight.detach()[index[valid]]
            b[valid] = lin.bias.detach()[index[valid]]
            return {"W": W, "b": b}
        st = self._enc_cache.get((lin.weight, lin.bias), build)
        return st["W"], st["b"]

    #: "auto" | "dense" | "prefilter" | "band" -- how the z bits are computed; the bits are identical on every path.
    #: dense: every latent from the exact-fp32 MFMA contraction.  prefilter: the fp16 candidate sweep lists the units near or
    #: above the sigmoid cutoff, latents inside the error band are re-evaluated exactly; the decoder walks the active units --
    #: pays off when few units fire per row.  band: an fp16 MFMA pass classifies EVERY latent and only the ~1 % inside the
    #: band are re-evaluated (qsae_encode_bits_band) -- for dense activations, where the lists of the prefilter overflow.
    #: auto: prefilter for large batches until a batch shows dense activations (more than half of its rows overflow their
    #: candidate lists, i.e. more than ~8 % of the units fire), then band (dense where the shape is not covered) for this model.
    bits_path = "auto"
    _PREFILTER_MIN_ROWS = 2048
    #: a ``training.FeatureActivity`` or None: when set, ``forward_train`` (never ``forward``) adds every batch's active units
    #: to it from the tensors it already holds; outputs and gradients are the same bits either way
    activity = None

    def resolved_bits_path(self, batch_rows: int) -> str:
        path = self.bits_path
        if path not in ("auto", "dense", "prefilter", "band"):
            raise ValueError(f"bits_path must be 'auto', 'dense', 'prefilter' or 'band', got {path!r}")
        W, _ = self._encoder_params()
        ok = ops.encode_bits_prefilter_supported(batch_rows, self.input_dim, W.shape[0])
        ok_band = ops.encode_bits_band_supported(batch_rows, self.input_dim, W.shape[0])
        if path == "auto":
            big = batch_rows >= self._PREFILTER_MIN_ROWS and W.shape[0] >= 2048
            if not big:
                path = "dense"
            elif getattr(self, "_dense_regime", False):
                path = "band" if ok_band else "dense"
            else:
                path = "prefilter" if ok else ("band" if ok_band else "dense")
        if path == "prefilter" and not ok:
            path = "dense"
        if path == "band" and not ok_band:
            path = "dense"
        return path

    def _prefilter_weights(self):
        W, b = self._encoder_params()
        if not hasattr(self, "_pref_cache"):
            self._pref_cache = PackedCache()
        lin = self.encoder.linear

        def build():
            self._dense_regime = False                     # new weights: probe the activation density again
            Wq, meta = ops.prefilter_pack_w(W, b)
            return {"Wq": Wq, "meta": meta}
        return self._pref_cache.get((lin.weight, lin.bias), build)

    def activation_bits(self, x, path: str = None) -> torch.Tensor:
        """int32-packed z = (sigmoid(encoder pre-activation) > 0.5) in packed hidden order."""
        with torch.no_grad():
            W, b = self._encoder_params()
            x = require_device_input(x, "x")
            path = path or self.resolved_bits_path(x.shape[0])
            if path in ("prefilter", "band"):
                pw = self._prefilter_weights()
                fn = ops.encode_bits_prefilter if path == "prefilter" else ops.encode_bits_band
                z, flagged = fn(x.float(), W, b, pw["Wq"], pw["meta"])
                self.last_flagged_rows = flagged
                if path == "prefilter" and flagged * 2 > x.shape[0]:   # the exact fallback of half the rows costs what the dense kernel does
                    self._dense_regime = True
                return z
            return ops.encode_bits(x, W, b)

    def forward(self, x):
        if torch.compiler.is_compiling():                  # one graph node: torch.ops.qsae.levels_sae_forward
            lin, dec = self.encoder.linear, self.decoder
            with torch.no_grad():
                groups, levels = torch.ops.qsae.levels_sae_forward(
                    x, [lin.weight, lin.bias, dec.weight, dec.weight_mirror, dec.bias], self._qsae_handle)
            return [groups[i] for i in range(self.n_bits)], [levels[i] for i in range(self.n_bits)]
        return self._forward_eager(x)

    def _forward_eager(self, x):
        with torch.no_grad():
            x = require_device_input(x, "x")
            path = self.resolved_bits_path(x.shape[0])
            return self.decoder.decode_bits(self.activation_bits(x, path))

    # -- training -------------------------------------------------------------------------------------------------
    #: "auto" | "dense" | "lists" -- how the backward sums the decoder-logit gradient dSum[h] = sum of G_i[r] over the rows
    #: r that activate unit h; read per call.  dense: one TN contraction of the z bits against G_i on the matrix pipe,
    #: whatever the density.  lists: per-unit row lists from a bit transpose of z, summed in list order -- work
    #: proportional to the number of active (row, unit) pairs.  auto: lists below LISTS_MAX_ACTIVE_FRACTION of active
    #: units over the same evenly spaced sample of rows that decode_bits decides on (a function of the batch alone).
    decoder_grad_path = "auto"
    #: measured at B = 8192, H = 32768, D = 512: the backward on lists takes 8.25 ms at 4.0 % active units and 9.59 ms at
    #: 6.6 %, on the dense contraction 8.4 to 8.6 ms at any density
    LISTS_MAX_ACTIVE_FRACTION = 0.04
    last_decoder_grad_path = None      # "dense" | "lists": what the previous forward_train resolved to (per model)

    def forward_train(self, x):
        """``(latent_groups, reconstruction_levels)`` as ``forward()`` returns them, same values bit for bit, every element
        with a ``grad_fn``: the forward the reference trains through (sae/quantized_matryoshka.py:47-143; the q_sae branch
        of training/trainer.py:88-112), whose backward runs the HIP gradient kernels (csrc/train_gemm.hip, csrc/train.hip;
        the table in DESIGN.md section 4.12).  ``loss.backward()`` fills the ``.grad`` of encoder.0.weight / .bias,
        decoder.weight / .weight_mirror / .bias (none for the bias without ``allow_bias``, as in the reference) and of
        ``x`` if it requires grad; then ``decoder.apply_secant_grad()``.

        The encoder pre-activation [B, H] is kept for the backward, which turns it into its own gradient in place: a
        second backward through the same graph raises.  Derived weights are keyed on the parameters' version counters,
        so an optimizer step is picked up by the next call."""
        path = self.decoder_grad_path
        if path not in ("auto", "dense", "lists"):
            raise ValueError(f"decoder_grad_path must be 'auto', 'dense' or 'lists', got {path!r}")
        D = self.input_dim
        if not ops.train_matryoshka_supported(D):
            raise ValueError(f"QuantizedMatryoshkaSAE.forward_train: the gradient kernels take input_dim a multiple of 4 up to "
                             f"4096 (got input_dim = {D})")
        if isinstance(x, torch.Tensor) and (x.dim() != 2 or x.shape[1] != D):
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        x = require_device_input(x, "x")
        if x.shape[0] < 1:
            raise ValueError("QuantizedMatryoshkaSAE.forward_train: the batch needs at least one row")
        Hp = sum(self.decoder.padded_sizes)
        if path == "lists" and not ops.train_bits_csr_supported(x.shape[0], Hp):
            raise ValueError(f"QuantizedMatryoshkaSAE.forward_train: decoder_grad_path = 'lists' takes batch * padded hidden "
                             f"size below 2^31 (got {x.shape[0]} * {Hp})")
        lin, dec = self.encoder.linear, self.decoder
        groups, levels = _MatryoshkaTrainStep.apply(self, path, x, lin.weight, lin.bias, dec.weight, dec.weight_mirror,
                                                    dec.bias)
        return [groups[i] for i in range(self.n_bits)], [levels[i] for i in range(self.n_bits)]

    def forward_submit(self, x, slot: int = 0):
        """Queue one forward without waiting for the GPU (see BinarySAE.forward_submit): the z bits of the fp16 candidate
        sweep are queued here (qsae_encode_bits_prefilter_submit); ``result()`` takes the count of rows that need the
        exact dense kernel, queues those, reads the batch's active-unit count, queues the decoder and returns
        ``(latent_groups, reconstruction_levels)``.  Batches in flight together need different ``slot`` numbers; models on the
        dense path compute eagerly."""
        with torch.no_grad():
            xd = require_device_input(x, "x")
            path = self.resolved_bits_path(xd.shape[0])
            if path not in ("prefilter", "band"):
                return _SubmittedMatryoshka(self, None, self.forward(xd), xd.shape[0], path)
            W, b = self._encoder_params()
            pw = self._prefilter_weights()
            pending = ops.encode_bits_prefilter_submit(xd.float(), W, b, pw["Wq"], pw["meta"], slot=slot, band=(path == "band"), owner=self._qsae_handle)
            return _SubmittedMatryoshka(self, pending, None, xd.shape[0], path)


class _SubmittedMatryoshka:
    def __init__(self, model, pending, outs, rows, path):
        self._model, self._pending, self._outs, self._rows, self._path = model, pending, outs, rows, path

    def result(self):
        with torch.no_grad():
            if self._pending is not None:
                m = self._model
                z = self._pending.finish()
                flagged = m.last_flagged_rows = self._pending.flagged_rows
                self._pending = None
                if self._path == "prefilter" and flagged * 2 > self._rows:
                    m._dense_regime = True
                self._outs = m.decoder.decode_bits(z)
            return self._outs


class _MatryoshkaTrainStep(torch.autograd.Function):
    """The QuantizedMatryoshkaSAE forward and its gradient (the table in DESIGN.md section 4.12).  Outputs: latent groups
    [n] and reconstruction levels [n, B, D] as two tensors (the caller hands out their elements).  The binarisation of the
    latent and of the decoder logits are straight-through estimators, so the encoder side of the gradient is dense:
    dz = scale <G_i, S> + gg_i / B for every unit of every row, dpre = dz p (1 - p), dW_enc = dpre^T x."""

    @staticmethod
    def forward(ctx, model, path, x, W_enc, b_enc, w, wm, bias):
        dec = model.decoder
        xf = as_f32c(x.detach())
        B = xf.shape[0]
        Wp, bp = model._encoder_params()
        st = dec.packed()
        # the dense exact-fp32 pre-activation, kept for the backward; its bits by the cutoff every bits path uses
        pre = ops.encode_dense(xf, Wp, bp)
        zbits = ops.train_pre_bits(pre)
        frac = dec.active_fraction(zbits)
        levels, counts = dec._decode_levels(zbits, dec.sparse_walk_possible(B) and frac < dec.SPARSE_MAX_ACTIVE_FRACTION)
        groups = (counts.to(torch.float64) / B).to(torch.float32)
        if path == "auto":
            path = "lists" if (frac < model.LISTS_MAX_ACTIVE_FRACTION and ops.train_bits_csr_supported(B, st["H"])) else "dense"
        tp = dec.train_pack()
        if model.activity is not None:
            model.activity.add_bits(zbits, tp["index"])      # the map analysis._stage_bits uses, as int32
        dec._train_ctx = {"zbits": zbits, "scale": st["scale"], "index": tp["index"], "rows": B,
                          "versions": (dec.weight._version, dec.weight_mirror._version)}
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, zbits, counts, st["scale"], tp["S"])
        ctx.pre = pre
        ctx.model, ctx.path, ctx.x_dtype = model, path, x.dtype
        ctx.sizes, ctx.index, ctx.valid = list(st["sizes"]), tp["index"], (st["index"] >= 0 if st["index"] is not None else None)
        model.last_decoder_grad_path = path
        return groups, levels

    @staticmethod
    def backward(ctx, g_groups, g_levels):
        xf, zbits, counts, scale, S = ctx.saved_tensors
        model = ctx.model
        dec = model.decoder
        need_x, need_W, need_b, need_w, need_wm, need_bias = ctx.needs_input_grad[2:8]
        sizes, Hp = ctx.sizes, zbits.shape[1] * 32
        G = None
        if g_levels is not None:
            G = as_f32c(g_levels)
        dx = dW = db = dw = dwm = dbias = None
        if need_x or need_W or need_b:
            if ctx.pre is None:
                raise RuntimeError("Trying to backward through QuantizedMatryoshkaSAE.forward_train a second time: the saved "
                                   "pre-activation was turned into its gradient in place by the first backward")
            dpre = ops.train_matryoshka_dpre(ctx.pre, G, g_groups, S, scale, sizes)
            ctx.pre = None
            Wp = model._encoder_params()[0] if need_x else None
            dx, dW, db = dense_encoder_backward(dpre, xf, Wp, need_x, need_W, need_b, ctx.x_dtype)
            del dpre                                       # 1 GiB at the full shape: gone before the decoder-logit gradients
            if ctx.valid is not None:                      # padded hidden order -> the model's units
                dW = dW[ctx.valid] if need_W else None
                db = db[ctx.valid] if need_b else None
        if need_w or need_wm:
            dsum = None
            if G is not None and ctx.path == "lists":
                n_entries = int(counts.sum().item())
                offsets, entries = ops.train_bits_csr(zbits, Hp, n_entries)
                dsum = ops.train_matryoshka_dsum_lists(offsets, entries, n_entries, G, sizes)
            elif G is not None:
                dsum = ops.train_matryoshka_dsum_dense(zbits, G, Hp, sizes)
            dw, dwm = ops.train_matryoshka_finish(dsum, scale, ctx.index, dec.weight.detach(), dec.weight_mirror.detach())
        if need_bias and dec.allow_bias:
            dbias = ops.train_col_sum(G[0]) if G is not None else torch.zeros_like(dec.bias)
        return (None, None, dx, dW, db, dw if need_w else None, dwm if need_wm else None, dbias)
