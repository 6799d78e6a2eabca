"""``Trainer``: the reference's epoch loop (training/trainer.py:18-261) on the GPU.

The constructor arguments, ``one_epoch`` and ``train`` are the reference's; the pieces of a step are this package's:
``ShuffledChunk`` supplies the DataLoader's batches from a device-resident chunk, ``model.forward_train`` carries the HIP
backward, ``trainer_loss`` the per-type loss, ``optim.Adam`` the step.  What differs from the reference, on purpose:

* ``bl_sae`` has no branch in the reference's loop, which never steps it; here it trains with ``mse`` + Adam, the recipe
  of tests/golden/train_blatent_loop.npz.
* ``t_sae`` without ``rigL`` raises ``ValueError`` at construction: the reference dies at its first step on
  ``update_mask(None, 0.7)`` (``None * float``).  An unknown ``sae_type`` raises ``ValueError`` as well (the reference goes
  on without a model).
* The chunk files are taken in sorted order; the reference takes them in ``os.listdir`` order, which the file system
  decides.
* ``wandb`` is imported only when it is installed and ``no_log`` is false.  Otherwise ``log_fn`` -- or, without one, the
  reference's ``print`` lines (its ``no_log`` formats; the ``bl_sae`` line is ``Loss=`` alone, the reference's fallback line
  names a sparsity loss that type does not have) -- receives the same metric dictionaries.  Metrics are computed on logging steps only
  (``batch_idx % log_every == 0``); no other step reads anything back or builds a [B, H] tensor for them.
* ``watch="all" | "parameters" | "gradients"`` with ``watch_freq`` (default 256, wandb's ``log_freq`` in the reference) gives
  the other half of what the reference logs: the histograms of ``wandb.watch`` for every parameter and gradient, from one
  kernel call (``ModelWatch``, csrc/watch.hip) on the steps with ``batch_idx % watch_freq == 0``.  They go to ``log_fn`` as
  ``TensorStats`` under wandb's keys (merged into the metrics of a step that is also a logging step), to wandb as
  ``wandb.Histogram``, and under ``no_log`` to one printed line per tensor.  The default ``None`` changes nothing.
* ``activity_window=W`` (rows; default ``None`` changes nothing) keeps per-feature firing counts on the GPU while the run
  trains (``FeatureActivity``, csrc/activity.hip): ``model.activity`` is set, every ``forward_train`` adds its batch from the
  tensors it already holds, and on logging steps -- the only steps that read anything back -- the metrics gain
  ``dead_features`` (not fired within the last W rows), ``dead_fraction``, ``never_fired``, ``silent_features`` (not fired since
  the previous logging step), ``mean_l0`` over that interval, ``count_octaves`` (34 bins of the interval's firing counts) and,
  for ``q_sae`` / ``rq_sae``, ``dead_features_level_{i}``; under ``no_log`` a second printed line follows the reference's.  The
  tracker lives as long as the Trainer, across ``one_epoch`` calls.  ``dead_neuron_threshold`` stays unread, as in the reference.
* ``resample_every=R`` (batches; ``baseline_sae`` and ``b_sae`` with ``activity_window`` only; default ``None`` changes
  nothing) revives dead units (``resample_dead``, csrc/resample.hip): on the steps with ``batch_idx % R == 0``, after the
  type's step sequence, the dead list of ``summary(activity_window, dead_list=True, advance=False)`` is rewritten from the
  batch just trained on, with the epoch's optimizer.  The uniforms come from a generator of the Trainer's own, seeded with
  ``resample_seed``; the default generator, and with it the loader's order, is not touched.  ``resample_scale`` is the
  encoder scale.  The report joins that step's metrics (``resampled_features``, ``resample_duplicates``, ...; one printed
  line under ``no_log``); these steps read the summary and the report back, no other step reads anything more than before.
* ``aux_k=K`` (``baseline_sae`` and ``b_sae`` with ``activity_window`` only; default ``None`` changes nothing) adds the AuxK
  loss of the top-k SAEs (``aux_k_loss``, csrc/auxk.hip): after the type's loss and its backward, the dead units of the
  tracker reconstruct the residual through their own top-K (K <= 64, clamped to the number of dead units) and
  ``aux_coef`` times the normalised error is backpropagated into the same ``.grad`` before the optimizer step.  The dead list
  is ``summary(activity_window, dead_list=True, advance=False).dead_indices``, taken every ``aux_refresh`` steps (default
  ``log_every``): a refresh is that summary's one host copy, between two refreshes nothing more is read back than before,
  and a list that has gone stale in between is fine.  Logging steps gain ``aux_loss`` and ``aux_units``.  Works together with
  ``resample_every``.
* ``nested_bounds="default" | [b_0, ..., b_{L-1}]`` (``baseline_sae`` and ``b_sae`` only; default ``None`` changes nothing) trains
  with the nested-dictionary objective (``nested_loss``, csrc/nested.hip): ``model.forward_train_nested`` gives one
  reconstruction per dictionary prefix ``[0, b_l)`` and the type's reconstruction term is summed over them; ``"default"`` is
  ``default_nested_bounds(hidden_dim)`` = ``[H/8, H/4, H/2, H]``.  Logging steps gain ``recon_loss_level_{l}``; ``loss`` and
  ``recon_loss`` are the sums.  The last level is the model's reconstruction, so ``aux_k``, ``resample_every`` and
  ``activity_window`` work as before.
* ``batch_topk=True`` (``baseline_sae`` and ``b_sae`` only; default ``False`` changes nothing) trains with BatchTopK
  (``BatchTopK``, csrc/batch_topk.hip): ``model.forward_train_batch_topk`` keeps the ``batch * k`` largest pre-activations of
  the whole batch, at most ``batch_topk_cap`` (default ``min(256, hidden_dim, 4 k)``) per row, and learns the inference
  threshold on the device.  Logging steps gain ``batch_topk/threshold``, ``batch_topk/saturated_rows`` and
  ``batch_topk/empty_rows``; nothing is read back between them.  ``aux_k``, ``resample_every`` and ``activity_window`` work
  as before.  Together with ``nested_bounds`` it raises: that keyword means the per-row top-k of ``forward_train_nested``, and
  the combination is asked for by name, with ``batch_topk_nested_bounds``.  ``batch_topk_dense=True`` (default ``False``; it
  needs ``batch_topk=True``) routes the step through ``model.forward_train_batch_topk_dense`` (csrc/batch_dense.hip), with
  ``batch_topk_nested_bounds`` through ``model.forward_train_nested_batch_topk_dense``: the same selection, bit for bit, taken
  from the pre-activations above a floor of ``batch_topk_floor_ratio`` (default ``BatchTopK.DEFAULT_FLOOR_RATIO``) times the
  last batch's smallest selected value instead of from every row's top-``cap`` list; the first step runs capped and seeds the
  floor.  Logging steps gain ``batch_topk/second_attempts`` (the batches so far whose floor was too high and that were
  selected again without one, on the device) and ``batch_topk/candidates_per_row``.
* ``batch_topk_nested_bounds="default" | [b_0, ..., b_{L-1}]`` (needs ``batch_topk=True``; default ``None`` changes nothing)
  trains the Matryoshka SAE as Bussmann et al. do, with BatchTopK: ``model.forward_train_nested_batch_topk`` gives one
  reconstruction per dictionary prefix from the batch-wide selection (csrc/nested_ragged.hip), the loss is ``nested_loss``,
  and AuxK takes the last level.  Logging steps gain ``recon_loss_level_{l}`` and ``l0_level_{l}``, the mean number of selected
  units below ``b_l`` per row (one small host copy; none on other steps), next to the ``batch_topk/*`` metrics.
* ``multi_topk="default" | [k_0, ..., k_{P-1}]`` (``baseline_sae`` and ``b_sae`` only; default ``None`` changes nothing) trains
  with the Multi-TopK objective of Gao et al. (``multi_topk_loss``, csrc/multi_topk.hip): ``model.forward_train_multi_topk``
  selects once at the widest point and gives one reconstruction per rank prefix; the objective is ``sum_p w_p * loss_p`` with
  ``multi_topk_weights`` (default 1 for the point equal to the model's top-k and 1/8 for the others: ``L(k) + L(4k) / 8``).
  ``"default"`` is ``default_multi_topk(top_k, hidden_dim)`` = ``[k, min(4 k, 256, H)]``.  The model's top-k must be one of
  the points: that point is the model's reconstruction for ``aux_k``, ``resample_every`` and the logged ``recon_loss``.
  Logging steps gain ``recon_loss_k{k_p}``.  Together with ``nested_bounds``, ``batch_topk`` or
  ``batch_topk_nested_bounds`` it raises: the combinations are not built.
* ``jumprelu=True`` (``baseline_sae`` and ``b_sae`` only; default ``False`` changes nothing) trains with JumpReLU
  (``JumpReLU``, csrc/jumprelu.hip): ``model.forward_train_jumprelu`` keeps, of every row's top-``jumprelu_cap`` list (default
  ``min(256, hidden_dim)``), the entries above their unit's learned threshold; the objective is the recipe's loss plus
  ``jumprelu_l0_coef`` (required: it has no sensible default) times the mean number of firing units per row, whose gradient
  is that constant; ``log_threshold`` joins every epoch's optimizer as a parameter group of its own.  ``jumprelu_bandwidth``
  is the width of the straight-through kernel; ``jumprelu_init`` is the initial threshold, or ``"calibrate"`` to set every
  threshold, on the first batch, to the smallest value BatchTopK would select there at the model's k.  Logging steps gain
  ``jumprelu/l0``, ``jumprelu/band_entries``, ``jumprelu/uncertified_rows``, ``jumprelu/saturated_rows`` and
  ``jumprelu/theta_min``; nothing is read back between them.  ``aux_k``, ``resample_every`` and ``activity_window`` work as
  with ``batch_topk``.  ``jumprelu_dense=True`` (default ``False``; it needs ``jumprelu=True``) routes the step through
  ``model.forward_train_jumprelu_dense`` (csrc/jump_dense.hip): the thresholds are applied to all pre-activations, no list
  and no certificate stand in between, ``jumprelu_cap`` is the widest row the step keeps; logging steps then report
  ``jumprelu/truncated_rows`` (rows with more firing units than the cap) in place of ``jumprelu/uncertified_rows`` and
  ``jumprelu/saturated_rows``, and no ``jumprelu/theta_min``.  Together with ``batch_topk``, ``nested_bounds``, ``batch_topk_nested_bounds`` or ``multi_topk`` it
  raises: the combinations are not built.
* ``grad_clip=c`` (a finite number > 0; every ``sae_type``; default ``None`` changes nothing) clips the joint gradient norm of
  every step to ``c`` (``optim.Adam(max_grad_norm=c)``, csrc/optim_recipe.hip): one norm call inside ``optimizer.step()``, over
  every parameter with a gradient -- the JumpReLU thresholds included -- and a coefficient word that the step kernels
  multiply the gradients by; ``.grad`` itself stays unscaled, so ``watch`` shows raw gradients.  Logging steps gain
  ``grad_norm``, ``grad_clip_coef`` and ``grad_clipped`` (one small host copy; no other step reads anything back).
  ``decoder_grad_projection=True`` (``baseline_sae`` only, the one model with unit-norm atoms; default ``False``) calls
  ``model.project_decoder_grad()`` between the backward (after ``apply_secant_grad`` / ``mask_grad`` and the watch
  collection) and ``optimizer.step()``: the decoder gradient loses its component along each atom.  ``ema_decay=d`` (a float
  in [0, 1); default ``None``) keeps an exponential moving average of every parameter in the step kernels
  (``optim.Adam(ema_decay=d, ema_state=trainer.ema_state)``); the Trainer owns the averages across the per-epoch optimizers,
  and ``train()`` saves them as a state dict next to the checkpoint, ``<model_path without .pth>_ema.pth``.
* ``model=`` hands in the model instead of building the reference's.  The reference builds
  ``BinarySAE(input_dim, hidden_dim, n_bits)``, where ``n_bits`` lands in ``gamma`` and the decoder keeps its default of 8
  bits; that call is kept.
"""
from __future__ import annotations

import importlib.util
import math
import os
import time
from typing import Callable, Optional

import torch

from .. import optim
from .. import torch_ops as ops
from ..sae import (BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, ResidualQuantizedSAE,
                   TernarySparseAutoencoder)
from ..sae.binary_latent import BinaryLatentSAE
from .batches import ShuffledChunk
from .loss import SAE_TYPES, trainer_loss
from .loss import _const as _loss_const
from .activity import FeatureActivity, activity_line
from .auxk import AUX_MAX_K, aux_k_loss
from .batch_topk import BatchTopK
from .jumprelu import JumpReLU
from .multi_topk import MULTI_TOPK_TYPES, default_multi_topk, default_multi_topk_weights, multi_topk_loss
from .nested import NESTED_TYPES, default_nested_bounds, nested_loss
from .resample import ResampleReport, resample_dead, resample_line
from .watch import WATCH_MODES, ModelWatch, watch_line

__all__ = ["Trainer", "model_path_for"]

CHUNK_PREFIX, CHUNK_SUFFIX = "the_pile_hidden_states_L3_", ".pt"
_BITS_IN_NAME = ("b_sae", "q_sae", "rq_sae")


def model_path_for(save_dir: str, sae_type: str, config: dict, rigL: bool) -> str:
    """The reference's checkpoint name (training/trainer.py:58) under ``save_dir``."""
    name = (sae_type + "_" + str(config["hidden_dim"]) + ("_rigL" if rigL else "")
            + (str(config["n_bits"]) + "_bits" if sae_type in _BITS_IN_NAME else "") + ".pth")
    return os.path.join(save_dir, name)


def _build_model(sae_type: str, config: dict) -> torch.nn.Module:
    D, H = config["input_dim"], config["hidden_dim"]
    if sae_type == "t_sae":
        return TernarySparseAutoencoder(D, H)
    if sae_type == "bl_sae":
        return BinaryLatentSAE(D, H)
    if sae_type == "b_sae":
        return BinarySAE(D, H, config["n_bits"])              # positional, as in the reference: n_bits lands in gamma
    if sae_type == "q_sae":
        return QuantizedMatryoshkaSAE(D, H, config["top_k"], config["gamma"], config["n_bits"])
    if sae_type == "rq_sae":
        return ResidualQuantizedSAE(D, H, config["top_k"], config["gamma"], config["n_bits"])
    return BaselineSparseAutoencoder(D, H)


class Trainer:
    def __init__(self, config, sae_type, rigL=False, no_log=False, proj_name=None, *, model: Optional[torch.nn.Module] = None,
                 dataset_dir: str = "dataset/", save_dir: str = "SAEs/", log_fn: Optional[Callable[[dict], None]] = None,
                 log_every: int = 100, watch: Optional[str] = None, watch_freq: int = 256,
                 activity_window: Optional[int] = None, resample_every: Optional[int] = None, resample_seed: int = 0,
                 resample_scale: float = 0.2, aux_k: Optional[int] = None, aux_coef: float = 1 / 32,
                 aux_refresh: Optional[int] = None, nested_bounds=None, batch_topk: bool = False,
                 batch_topk_cap: Optional[int] = None, batch_topk_nested_bounds=None, multi_topk=None,
                 multi_topk_weights=None, jumprelu: bool = False, jumprelu_l0_coef: Optional[float] = None,
                 jumprelu_cap: Optional[int] = None, jumprelu_bandwidth: float = 1e-3, jumprelu_init=None,
                 jumprelu_dense: bool = False, batch_topk_dense: bool = False,
                 batch_topk_floor_ratio: Optional[float] = None, grad_clip: Optional[float] = None,
                 decoder_grad_projection: bool = False, ema_decay: Optional[float] = None):
        if sae_type not in SAE_TYPES:
            raise ValueError(f"unknown sae_type {sae_type!r}; expected one of {', '.join(SAE_TYPES)}")
        if sae_type == "t_sae" and not rigL:
            raise ValueError("t_sae trains with rigL=True only: its step calls decoder.update_mask(f_decay, 0.7), and f_decay "
                             "is set by the rigL schedule (the reference fails on None * float at the first step)")
        if int(log_every) < 1:
            raise ValueError(f"log_every = {log_every}")
        if watch is not None and watch not in WATCH_MODES:
            raise ValueError(f"watch = {watch!r}; expected None or one of {', '.join(WATCH_MODES)}")
        if int(watch_freq) < 1:
            raise ValueError(f"watch_freq = {watch_freq}")
        if activity_window is not None and int(activity_window) < 1:
            raise ValueError(f"activity_window = {activity_window}; expected None or a number of rows >= 1")
        if resample_every is not None:
            if int(resample_every) < 1:
                raise ValueError(f"resample_every = {resample_every}; expected None or a number of batches >= 1")
            if activity_window is None:
                raise ValueError("resample_every needs activity_window: the dead list comes from the activity tracker")
            if sae_type not in ("baseline_sae", "b_sae"):
                raise ValueError(f"resample_every: resampling is built for baseline_sae and b_sae, the two top-k models; got "
                                 f"{sae_type!r}")
        if aux_k is not None:
            if not 1 <= int(aux_k) <= AUX_MAX_K:
                raise ValueError(f"aux_k = {aux_k}; expected None or a number of units from 1 to {AUX_MAX_K}, the subset top-k "
                                 "kernel's limit")
            if activity_window is None:
                raise ValueError("aux_k needs activity_window: the dead list comes from the activity tracker")
            if sae_type not in ("baseline_sae", "b_sae"):
                raise ValueError(f"aux_k: the auxiliary loss is built for baseline_sae and b_sae, the two top-k models; got "
                                 f"{sae_type!r}")
            if aux_refresh is not None and int(aux_refresh) < 1:
                raise ValueError(f"aux_refresh = {aux_refresh}; expected None or a number of batches >= 1")
        if nested_bounds is not None and sae_type not in NESTED_TYPES:
            raise ValueError(f"nested_bounds: the nested objective is built for baseline_sae and b_sae, the two top-k models; "
                             f"got {sae_type!r}")
        if batch_topk and sae_type not in NESTED_TYPES:
            raise ValueError(f"batch_topk: the batch-wide selection is built for baseline_sae and b_sae, the two top-k models; "
                             f"got {sae_type!r}")
        if batch_topk and nested_bounds is not None:
            raise ValueError("batch_topk together with nested_bounds: nested_bounds selects k units per row; the nested levels "
                             "of a batch-wide selection are asked for with batch_topk_nested_bounds")
        if batch_topk_nested_bounds is not None and not batch_topk:
            raise ValueError("batch_topk_nested_bounds needs batch_topk=True (nested_bounds is the keyword of the per-row top-k)")
        if batch_topk_cap is not None and not batch_topk:
            raise ValueError("batch_topk_cap needs batch_topk=True")
        if batch_topk_dense and not batch_topk:
            raise ValueError("batch_topk_dense needs batch_topk=True")
        if batch_topk_floor_ratio is not None and not batch_topk_dense:
            raise ValueError("batch_topk_floor_ratio needs batch_topk_dense=True")
        if multi_topk is not None:
            if sae_type not in MULTI_TOPK_TYPES:
                raise ValueError(f"multi_topk: the Multi-TopK objective is built for baseline_sae and b_sae, the two top-k models; "
                                 f"got {sae_type!r}")
            if nested_bounds is not None or batch_topk or batch_topk_nested_bounds is not None:
                raise ValueError("multi_topk together with nested_bounds, batch_topk or batch_topk_nested_bounds: the "
                                 "combinations are not built; choose one objective")
        elif multi_topk_weights is not None:
            raise ValueError("multi_topk_weights needs multi_topk")
        if jumprelu:
            if sae_type not in NESTED_TYPES:
                raise ValueError(f"jumprelu: the per-unit thresholds are built for baseline_sae and b_sae, the two top-k models; "
                                 f"got {sae_type!r}")
            for name, given in (("batch_topk", batch_topk), ("nested_bounds", nested_bounds is not None),
                                ("batch_topk_nested_bounds", batch_topk_nested_bounds is not None),
                                ("multi_topk", multi_topk is not None)):
                if given:
                    raise ValueError(f"jumprelu together with {name}: the combination is not built; choose one objective")
            if jumprelu_l0_coef is None:
                raise ValueError("jumprelu needs jumprelu_l0_coef, the weight of the L0 penalty: it depends on the scale of the "
                                 "data and has no default")
            if not (math.isfinite(float(jumprelu_l0_coef)) and float(jumprelu_l0_coef) >= 0):
                raise ValueError(f"jumprelu_l0_coef = {jumprelu_l0_coef}; expected a finite number >= 0")
            if isinstance(jumprelu_init, str) and jumprelu_init != "calibrate":
                raise ValueError(f"jumprelu_init = {jumprelu_init!r}; expected None, a threshold > 0 or 'calibrate'")
        else:
            for name, given in (("jumprelu_l0_coef", jumprelu_l0_coef), ("jumprelu_cap", jumprelu_cap),
                                ("jumprelu_init", jumprelu_init)):
                if given is not None:
                    raise ValueError(f"{name} needs jumprelu=True")
            if jumprelu_dense:
                raise ValueError("jumprelu_dense needs jumprelu=True")
        if grad_clip is not None:
            if isinstance(grad_clip, bool) or not isinstance(grad_clip, (int, float)) or \
                    not (math.isfinite(grad_clip) and grad_clip > 0):
                raise ValueError(f"grad_clip = {grad_clip!r}; expected None or a finite number > 0")
        if decoder_grad_projection and sae_type != "baseline_sae":
            raise ValueError(f"decoder_grad_projection: the projection is for baseline_sae, the one model with unit-norm atoms; "
                             f"got {sae_type!r}")
        if ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= ema_decay < 1.0:
                raise ValueError(f"ema_decay = {ema_decay!r}; expected None or a float in [0, 1)")
        self.config = config
        self.sae_type = sae_type
        #: the recipe around the optimizer step: the clip value, whether the decoder gradient is projected, the decay
        self.grad_clip = grad_clip
        self.decoder_grad_projection = bool(decoder_grad_projection)
        self.ema_decay = ema_decay
        #: parameter -> its exponential moving average, shared by every epoch's optimizer (None without ``ema_decay``)
        self.ema_state = {} if ema_decay is not None else None
        self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.model = (model if model is not None else _build_model(sae_type, config)).to(self.device)
        if sae_type == "b_sae":
            self.scale_factor = torch.pow(2, torch.arange(self.config["n_bits"])).to(self.device)
            self.scale_factor = self.scale_factor / self.scale_factor.sum().float()
        self.epoch = 0
        self.trained_batches = []                             # per one_epoch call: the batch_idx of every batch trained on
        self.dataset_dir, self.save_dir = dataset_dir, save_dir
        self.chunk_files = sorted(f for f in os.listdir(dataset_dir) if f.startswith(CHUNK_PREFIX) and f.endswith(CHUNK_SUFFIX))

        # rigL settings:
        self.rigL = rigL
        self.connection_fraction_to_update = 0.3
        self.f_decay = None

        self.model_path = model_path_for(save_dir, sae_type, config, rigL)

        self.no_log = no_log
        self.log_fn = log_fn
        self.log_every = int(log_every)
        self._wandb = None
        if not self.no_log and log_fn is None and importlib.util.find_spec("wandb") is not None:
            import wandb
            self._wandb = wandb
            wandb.init(project=proj_name, config=config)
            wandb.watch(self.model, log="all", log_freq=256)
        self.watch_freq = int(watch_freq)
        self._watch = ModelWatch(self.model, log=watch) if watch is not None else None
        self._watch_due, self._watched = False, None          # this step collects / what it collected
        self.activity_window = int(activity_window) if activity_window is not None else None
        self.activity = None
        if self.activity_window is not None:
            self.activity = self.model.activity = FeatureActivity.for_model(self.model)
        self.resample_every = int(resample_every) if resample_every is not None else None
        self.resample_scale, self._resample_seed = float(resample_scale), int(resample_seed)
        self._resample_rng = None                             # made on the first resampling step, on the model's device
        self.aux_k = int(aux_k) if aux_k is not None else None
        self.aux_coef = float(aux_coef)
        self.aux_refresh = int(aux_refresh) if aux_refresh is not None else self.log_every
        self._aux_units, self._aux_steps, self._aux_loss = None, 0, None   # the dead list in use, steps taken with it, last loss
        #: the bounds of the nested objective, from ``nested_bounds`` or (with BatchTopK) ``batch_topk_nested_bounds``, or None
        self.nested_bounds = None
        for name, given in (("nested_bounds", nested_bounds), ("batch_topk_nested_bounds", batch_topk_nested_bounds)):
            if given is not None:
                H = self.model.encoder.linear.weight.shape[0]
                if isinstance(given, str):
                    if given != "default":
                        raise ValueError(f"{name} = {given!r}; expected None, 'default' or a list of bounds")
                    given = default_nested_bounds(H)
                self.nested_bounds = ops.nested_bounds(given, H, f"Trainer: {name}")
        #: the BatchTopK controller (k = the model's top-k), or None
        self.batch_topk = None
        if batch_topk:
            self.batch_topk = BatchTopK(self.model, cap=batch_topk_cap, dense=bool(batch_topk_dense),
                                        floor_ratio=batch_topk_floor_ratio)
        #: whether BatchTopK selects through the dense encoder (csrc/batch_dense.hip)
        self.batch_topk_dense = bool(batch_topk_dense)
        #: the points of the Multi-TopK objective, their weights and the index of the point equal to the model's top-k, or None
        self.multi_topk = self.multi_topk_weights = self._multi_topk_own = None
        if multi_topk is not None:
            H = self.model.encoder.linear.weight.shape[0]
            own = self.model._own_top_k()
            if isinstance(multi_topk, str):
                if multi_topk != "default":
                    raise ValueError(f"multi_topk = {multi_topk!r}; expected None, 'default' or a list of points")
                multi_topk = default_multi_topk(own, H)
            try:
                K = int(list(multi_topk)[-1])
            except (TypeError, IndexError, ValueError):
                raise ValueError(f"Trainer: multi_topk: ks must be a non-empty sequence of ints, got {multi_topk!r}") from None
            if K > H:
                raise ValueError(f"Trainer: multi_topk: ks = {list(multi_topk)} ends above hidden_dim = {H}")
            self.multi_topk = ops.multik_points(multi_topk, K, "Trainer: multi_topk")
            if own not in self.multi_topk:
                raise ValueError(f"Trainer: multi_topk: ks = {self.multi_topk} must hold the model's top-k = {own}: that point is "
                                 "the model's reconstruction")
            self._multi_topk_own = self.multi_topk.index(own)
            if multi_topk_weights is None:
                multi_topk_weights = default_multi_topk_weights(self.multi_topk, own)
            try:
                self.multi_topk_weights = [float(w) for w in multi_topk_weights]
            except (TypeError, ValueError):
                raise ValueError(f"multi_topk_weights = {multi_topk_weights!r}; expected one number per point") from None
            if len(self.multi_topk_weights) != len(self.multi_topk) or \
                    not all(math.isfinite(w) and w >= 0 for w in self.multi_topk_weights):
                raise ValueError(f"multi_topk_weights = {multi_topk_weights!r}; expected {len(self.multi_topk)} finite numbers "
                                 ">= 0, one per point")

        #: the JumpReLU controller (its log_threshold joins every epoch's optimizer as a group of its own), or None
        self.jumprelu = None
        self.jumprelu_l0_coef = float(jumprelu_l0_coef) if jumprelu else None
        self._jumprelu_calibrate = False                       # calibrate on the next batch trained on
        self.jumprelu_dense = bool(jumprelu_dense)
        if jumprelu:
            calibrate = isinstance(jumprelu_init, str)
            self.jumprelu = JumpReLU(self.model, cap=jumprelu_cap, bandwidth=jumprelu_bandwidth,
                                     init_threshold=None if calibrate else jumprelu_init)
            self._jumprelu_calibrate = calibrate
            if calibrate and self.model._own_top_k() > self.jumprelu.cap:
                raise ValueError(f"jumprelu_init = 'calibrate': the model's top-k = {self.model._own_top_k()} exceeds "
                                 f"jumprelu_cap = {self.jumprelu.cap}")

    # ---- one step ------------------------------------------------------------------------------------------------
    def _forward(self, batch, want_latent: bool):
        if self.nested_bounds is not None and self.batch_topk is not None:
            step = self.model.forward_train_nested_batch_topk_dense if self.batch_topk_dense else \
                self.model.forward_train_nested_batch_topk
            return step(batch, self.batch_topk, self.nested_bounds, dense_latent=want_latent)
        if self.nested_bounds is not None:
            return self.model.forward_train_nested(batch, self.nested_bounds, dense_latent=want_latent)
        if self.multi_topk is not None:
            return self.model.forward_train_multi_topk(batch, self.multi_topk, dense_latent=want_latent)
        if self.batch_topk is not None:
            step = self.model.forward_train_batch_topk_dense if self.batch_topk_dense else self.model.forward_train_batch_topk
            return step(batch, self.batch_topk, dense_latent=want_latent)
        if self.jumprelu is not None:
            step = self.model.forward_train_jumprelu_dense if self.jumprelu_dense else self.model.forward_train_jumprelu
            return step(batch, self.jumprelu, dense_latent=want_latent)
        if self.sae_type in ("b_sae", "baseline_sae"):
            return self.model.forward_train(batch, dense_latent=want_latent)
        return self.model.forward_train(batch)

    def _step(self, optimizer, batch, log_step: bool):
        """forward, loss, backward and the type's step sequence (training/trainer.py:88-173) -> (outputs, losses).
        On a watch step (``self._watch_due``, set by one_epoch) the distributions are collected into ``self._watched`` right
        after the backward, where wandb's hooks see the tensors: the parameters as the forward used them, the gradients as
        autograd left them (before apply_secant_grad / mask_grad and the optimizer step)."""
        st, model = self.sae_type, self.model
        if self._jumprelu_calibrate:                           # the first batch: thresholds at the model's own k (on the device)
            self.jumprelu.calibrate(batch, model._own_top_k())
            self._jumprelu_calibrate = False
        outputs = self._forward(batch, log_step)
        optimizer.zero_grad(set_to_none=True)
        if self.nested_bounds is not None:
            losses = nested_loss(st, outputs, batch, self.config)
        elif self.multi_topk is not None:
            losses = multi_topk_loss(st, outputs, batch, self.config, self.multi_topk_weights)
        elif self.jumprelu is not None:                        # l0 is linear in the objective: its gradient is the coefficient
            l0, outputs = outputs[-1], outputs[:-1]
            losses = trainer_loss(st, outputs, batch, self.config,
                                  extra=[(l0, _loss_const(batch.device, tuple(l0.shape), self.jumprelu_l0_coef))])
        else:
            losses = trainer_loss(st, outputs, batch, self.config)
        if self.aux_k is not None:                             # (nested: the last level is the model's reconstruction;
            if self.multi_topk is not None:                    #  Multi-TopK: the point at the model's own top-k)
                self._aux_backward(batch, outputs[1][self._multi_topk_own])
            else:
                self._aux_backward(batch, outputs[1] if self.nested_bounds is None else outputs[1][-1])
        self._watched = self._watch.collect() if self._watch_due else None
        if st == "q_sae":
            model.decoder.apply_secant_grad()
        elif st == "rq_sae":
            model.apply_secant_grad()
        elif st == "t_sae":
            model.decoder.mask_grad()
        if self.decoder_grad_projection:
            model.project_decoder_grad()
        optimizer.step()
        if st == "t_sae":
            model.decoder.update_mask(self.f_decay, 0.7)
        elif st == "baseline_sae":
            model.normalize_decoder_weights()
        return outputs, losses

    def _aux_backward(self, batch, recon) -> None:
        """The AuxK term of a step: its loss over the dead list in use, backpropagated into the ``.grad`` the type's loss
        has just filled.  The list is refreshed every ``aux_refresh`` steps (the summary's one host copy)."""
        if self._aux_steps % self.aux_refresh == 0:
            self._aux_units = self.activity.summary(self.activity_window, dead_list=True, advance=False).dead_indices
        self._aux_steps += 1
        self._aux_loss = None
        if self._aux_units.shape[0] > 0:
            self._aux_loss = aux_k_loss(self.model, batch, recon, self._aux_units, self.aux_k, self.aux_coef)
            self._aux_loss.backward()

    # ---- metrics (logging steps only) --------------------------------------------------------------------------------------
    def _plane_magnitudes(self):
        """mag_MSB, mag_LSB: decoder.weight[:, n-1::n].abs().mean() and [:, 0::n] for n = config["n_bits"], from the
        per-bit-plane sums of |logit| that ops.quantization_error yields."""
        dec, n = self.model.decoder, int(self.config["n_bits"])
        N = dec.n_bits
        if N % n != 0:                                         # the stride does not follow the planes: slice as the reference does
            w = dec.weight.detach()
            return w[:, n - 1::n].abs().mean().item(), w[:, 0::n].abs().mean().item()
        H = dec.weight.shape[0]
        D = dec.weight.shape[1] // N
        result, _ = ops.quantization_error(dec.weight.detach(), D, N, float(dec.quantization_step), 0.0)
        planes = result[16:16 + N].tolist()
        per = H * D * (N // n)
        return sum(planes[n - 1::n]) / per, sum(planes[0::n]) / per

    def _metrics(self, outputs, losses) -> dict:
        st, cfg = self.sae_type, self.config
        lv = losses.tolist()
        levels = {}
        if self.nested_bounds is not None:                     # the objective is the sum over the levels
            levels = {f"recon_loss_level_{i}": v for i, v in enumerate(lv)}
            lv = [sum(lv)]
        if self.multi_topk is not None:                        # the objective is the weighted sum over the points
            levels = {f"recon_loss_k{k}": v for k, v in zip(self.multi_topk, lv)}
            levels["recon_loss"] = lv[self._multi_topk_own]
            lv = [sum(w * v for w, v in zip(self.multi_topk_weights, lv))]
        if st == "b_sae":
            latent, _, pol = outputs
            pol = pol.item()
            msb, lsb = self._plane_magnitudes()
            return {"loss": lv[0] + cfg["polarize_lambda"] * pol, "recon_loss": lv[0], "polarize_loss": pol,
                    "activated_neurons": torch.mean(latent.sum(dim=-1)).item(), "mag_MSB": msb, "mag_LSB": lsb, **levels}
        if st in ("q_sae", "rq_sae"):
            n = cfg["n_bits"]
            l0 = [g.item() for g in outputs[0]]
            lam = cfg["sparsity_lambda"]
            if st == "q_sae":
                d = {f"recon_loss_group_{i}": lv[i] for i in range(n)}
                d["recon_loss_total"] = sum(lv)
                sparsity = sum(l0) * lam
            else:
                d = {f"recon_loss_group_{i}": lv[i] / 4 ** i for i in range(n)}
                sparsity = sum(l0[i] * lam * w for i, w in enumerate((1.0, 2.5, 4.0, 8.0)[:len(l0)]))
            d.update({f"L0 of latent_group_{i}": l0[i] for i in range(n)})
            d["sparsity loss"] = sparsity
            return d
        return {"loss": lv[0], **levels}

    def _aux_metrics(self) -> dict:
        """What a logging step adds with ``aux_k``: the step's auxiliary loss (0.0 when no unit was dead) and the length of the
        dead list it ran over"""
        return {"aux_loss": self._aux_loss.item() if self._aux_loss is not None else 0.0,
                "aux_units": int(self._aux_units.shape[0])}

    def _batch_topk_metrics(self) -> dict:
        """What a logging step adds with ``batch_topk``: the threshold and the last selection's saturated and empty rows (one
        host copy of five words; no other step reads them)"""
        b = self.batch_topk.summary()
        d = {"batch_topk/threshold": b["threshold"], "batch_topk/saturated_rows": b["saturated_rows"],
             "batch_topk/empty_rows": b["empty_rows"]}
        if self.batch_topk_dense:
            # (no dense report yet: only the capped step that seeds the floor has run, over every row's whole list)
            e = self.batch_topk.dense_summary() if self.batch_topk.report_dense is not None else \
                {"second_attempts": 0, "candidates_per_row": float(self.batch_topk.cap)}
            d.update({"batch_topk/second_attempts": e["second_attempts"], "batch_topk/candidates_per_row": e["candidates_per_row"]})
        if self.nested_bounds is not None:                     # the mean selected units per row below every bound (one copy)
            l0 = self.batch_topk.level_counts.to(torch.float64).mean(dim=1).tolist()
            d.update({f"l0_level_{l}": v for l, v in enumerate(l0)})
        return d

    def _jumprelu_metrics(self) -> dict:
        """What a logging step adds with ``jumprelu``: the last selection's report (one host copy of six words; no other step
        reads it)"""
        j = self.jumprelu.summary()
        if self.jumprelu_dense:
            return {"jumprelu/l0": j["l0"], "jumprelu/band_entries": j["band_entries"],
                    "jumprelu/truncated_rows": j["truncated_rows"], "jumprelu/empty_rows": j["empty_rows"]}
        return {"jumprelu/l0": j["l0"], "jumprelu/band_entries": j["band_entries"],
                "jumprelu/uncertified_rows": j["uncertified_rows"], "jumprelu/saturated_rows": j["saturated_rows"],
                "jumprelu/theta_min": j["theta_min"]}

    def _activity_metrics(self, summary) -> dict:
        """What a logging step adds with ``activity_window``: the summary that ends the interval since the previous one"""
        d = {"dead_features": summary.dead, "dead_fraction": summary.dead_fraction, "never_fired": summary.never,
             "silent_features": summary.silent, "mean_l0": summary.mean_l0, "count_octaves": list(summary.octaves)}
        if self.sae_type in ("q_sae", "rq_sae"):
            d.update({f"dead_features_level_{i}": lv.dead for i, lv in enumerate(summary.levels)})
        return d

    def _print_line(self, batch_idx: int, m: dict) -> str:
        """The reference's print line of a logging step under no_log (training/trainer.py:213-230), from the metrics"""
        st, n = self.sae_type, self.config["n_bits"]
        if st == "b_sae":
            return (f"Batch {batch_idx}: Loss={m['loss']:.4f}, recon_loss={m['recon_loss']:.4f}, "
                    f"polarize_loss={m['polarize_loss']:.4f}, activated_neurons={m['activated_neurons']:.4f}, "
                    f"mag_MSB={m['mag_MSB']:.4f}, mag_LSB={m['mag_LSB']:.4f}")
        if st in ("q_sae", "rq_sae"):
            scale = 4 if st == "rq_sae" else 1                 # the rq_sae line shows group i divided by 4^i, loss_total does not
            loss_total = sum(m[f"recon_loss_group_{i}"] * scale ** i for i in range(n)) + m["sparsity loss"]
            recon = ", ".join(f"recon_loss_group_{i}={m[f'recon_loss_group_{i}']:.4f}" for i in range(n))
            l0 = ", ".join(f"L0_of_latent_group_{i}={m[f'L0 of latent_group_{i}']:.4f}" for i in range(n))
            return f"Batch {batch_idx}: {recon}, recon_loss_total={loss_total:.4f}, {l0}"
        return f"Batch {batch_idx}: Loss={m['loss']:.4f}"

    def _resample(self, optimizer, batch):
        """A resampling step: the dead units of the tracker, rewritten from the batch just trained on -> the report (all
        zeros, with nothing launched, when no unit is dead)"""
        summary = self.activity.summary(self.activity_window, dead_list=True, advance=False)
        if summary.dead == 0:
            return ResampleReport()
        if self._resample_rng is None:
            self._resample_rng = torch.Generator(device=self.device)
            self._resample_rng.manual_seed(self._resample_seed)
        return resample_dead(self.model, summary.dead_indices, batch, optimizer=optimizer, activity=self.activity,
                             generator=self._resample_rng, encoder_scale=self.resample_scale)

    def _log(self, batch_idx: int, metrics: Optional[dict], watched: Optional[dict] = None, activity=None, resampled=None) -> None:
        """metrics: the scalars of a logging step or None; watched: the distributions of a watch step or None; activity: the
        ActivitySummary of a logging step with ``activity_window`` or None; resampled: the ResampleReport of a resampling
        step or None.  A step that is several of these hands log_fn (or wandb) one dictionary."""
        if activity is not None:
            metrics = {**(metrics or {}), **self._activity_metrics(activity)}
        printing = self.log_fn is None and self._wandb is None
        if resampled is not None and not printing:
            metrics = {**(metrics or {}), **resampled.metrics()}
        if self.log_fn is not None:
            self.log_fn({**(metrics or {}), **(watched or {})})
        elif self._wandb is not None:
            hists = {k: self._wandb.Histogram(np_histogram=s.np_histogram()) for k, s in (watched or {}).items()}
            self._wandb.log({**(metrics or {}), **hists})
        else:
            if metrics is not None:
                print(self._print_line(batch_idx, metrics))
            if activity is not None:
                print(activity_line(activity))
            if resampled is not None:
                print(f"Batch {batch_idx}:" + resample_line(resampled))
            if watched is not None:
                print(f"Batch {batch_idx}: watch")
                for key, s in watched.items():
                    print(watch_line(key, s))

    def _make_optimizer(self):
        """An epoch's optimizer: a fresh Adam, as in the reference, with the recipe's options and the Trainer's averages"""
        optimizer = optim.Adam(self.model.parameters(), lr=self.config["lr"], model=self.model, max_grad_norm=self.grad_clip,
                               ema_decay=self.ema_decay, ema_state=self.ema_state)
        if self.jumprelu is not None:
            optimizer.add_param_group({"params": [self.jumprelu.log_threshold]})
        return optimizer

    # ---- the reference's interface -----------------------------------------------------------------------------------------
    def one_epoch(self, dataset, dead_neuron_threshold=0.2, no_log=False, rigL=False, f_decay=None):
        """One pass over a chunk: ``dataset`` is a ``ShuffledChunk``, a ``HiddenStatesTorchDataset``, a chunk file or the
        chunk tensor.  A fresh Adam per call, as in the reference.  The remaining arguments are the reference's and, as
        there, not read."""
        if self.device.type != "cuda":
            raise RuntimeError("Trainer.one_epoch: quantizedsae_amd runs on MI355X only (no CPU fallback exists)")
        chunk = dataset if isinstance(dataset, ShuffledChunk) else ShuffledChunk(dataset, self.config["batch_size"], self.device)
        optimizer = self._make_optimizer()
        self.trained_batches.append([])
        told = 0                                               # skipped batches announced so far, in batch order

        def announce(up_to):
            nonlocal told
            skipped = chunk.last_plan.skipped
            while told < len(skipped) and (up_to is None or skipped[told] < up_to):
                print(f"Batch {skipped[told]} contains NaN values before forward pass!")
                told += 1
        for batch_idx, batch in chunk.epoch():
            announce(batch_idx)
            self.trained_batches[-1].append(batch_idx)
            log_step = batch_idx % self.log_every == 0
            watch_step = self._watch is not None and batch_idx % self.watch_freq == 0
            self._watch_due = watch_step
            outputs, losses = self._step(optimizer, batch, log_step)
            resampled = None
            if self.resample_every is not None and batch_idx % self.resample_every == 0:
                resampled = self._resample(optimizer, batch)
            if log_step or watch_step or resampled is not None:
                summary = self.activity.summary(self.activity_window) if (log_step and self.activity is not None) else None
                metrics = self._metrics(outputs, losses) if log_step else None
                if log_step and self.aux_k is not None:
                    metrics.update(self._aux_metrics())
                if log_step and self.batch_topk is not None:
                    metrics.update(self._batch_topk_metrics())
                if log_step and self.jumprelu is not None:
                    metrics.update(self._jumprelu_metrics())
                if log_step and self.grad_clip is not None:
                    clip = optimizer.clip_report()
                    metrics.update({"grad_norm": clip.norm, "grad_clip_coef": clip.coef, "grad_clipped": int(clip.clipped)})
                self._log(batch_idx, metrics, self._watched, summary, resampled)
        announce(None)
        chunk.check()
        return self.model

    @property
    def ema_path(self) -> str:
        """Where ``train()`` saves the averaged weights: beside the checkpoint"""
        root = self.model_path[:-len(".pth")] if self.model_path.endswith(".pth") else self.model_path
        return root + "_ema.pth"

    def ema_state_dict(self) -> dict:
        """The model's state dict with every averaged parameter replaced by its average (``ema_decay`` set; a parameter that has
        not been stepped yet keeps its value)"""
        if self.ema_state is None:
            raise ValueError("ema_state_dict needs ema_decay")
        averaged = {name: self.ema_state[p] for name, p in self.model.named_parameters() if p in self.ema_state}
        return {name: averaged[name].detach().clone() if name in averaged else value.detach().clone()
                for name, value in self.model.state_dict().items()}

    def train(self):
        total_start = time.perf_counter()
        for epoch, f in enumerate(self.chunk_files):
            if epoch > 100:
                break
            print(f"Training on {f}:")
            self.epoch = epoch
            if self.rigL:
                self.f_decay = self.connection_fraction_to_update / 2 * (1 + math.cos(epoch * math.pi / len(self.chunk_files)))
                self.model.decoder.update_mask(self.f_decay, 0.7)
            self.one_epoch(os.path.join(self.dataset_dir, f), dead_neuron_threshold=0.2, no_log=self.no_log, rigL=self.rigL,
                           f_decay=self.f_decay)
        if self._wandb is not None:
            self._wandb.finish()
        os.makedirs(os.path.dirname(self.model_path) or ".", exist_ok=True)
        torch.save(self.model.state_dict(), self.model_path)
        if self.ema_state is not None:
            torch.save(self.ema_state_dict(), self.ema_path)
        print(f"Training completed. Model been saved to {self.model_path}.")
        total_time = time.perf_counter() - total_start
        print(f"Total training time: {total_time:.2f} seconds")
