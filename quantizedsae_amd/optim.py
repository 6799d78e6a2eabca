"""``quantizedsae_amd.optim.Adam``: the optimizer step in HIP (csrc/optim.hip).

A drop-in for ``torch.optim.Adam(model.parameters(), lr=...)`` (training/trainer.py:68): every parameter is stepped by one
pass of ``torch.ops.qsae.adam_step``.  With ``model=`` set to one of the top-k models (BinarySAE, BaselineSparseAutoencoder)
the encoder's weight and bias are stepped together by ``torch.ops.qsae.adam_step_prefilter``, which also leaves the fp16
candidate-pass copy of the new weights; the optimizer installs it in the model's cache, so the next forward does not
rebuild it.  The state (``step``, ``exp_avg``, ``exp_avg_sq``) has the names, dtypes and placement of torch's non-capturable
Adam: state dicts go back and forth between the two.

Around the step, the recipe of the top-k SAE papers (csrc/optim_recipe.hip), each piece in the pass
that already touches the data: ``max_grad_norm`` clips the joint gradient norm -- one ``grad_norm`` call leaves the coefficient
as a device word that every step kernel multiplies the gradient by -- and ``ema_decay`` keeps an exponential moving average
of the weights as one more stream of the step kernel.  Without them ``step()`` calls exactly the ops it called before.
"""
from __future__ import annotations

import contextlib
import math
from collections import namedtuple
from typing import Optional

import torch

from . import torch_ops as ops
from .sae.topk import TopKCore

__all__ = ["Adam", "ClipReport"]

#: ``Adam.clip_report()``: the joint gradient norm of the last step (fp64), the coefficient its kernels multiplied the gradients
#: by, whether that was a clip, and every tensor's sum of squares in the order of the param groups
ClipReport = namedtuple("ClipReport", ["norm", "coef", "clipped", "per_tensor"])

# options of torch.optim.Adam that have no kernel here; kept in the param groups (off) so that state dicts stay
# interchangeable
_UNSUPPORTED = ("weight_decay", "amsgrad", "maximize", "capturable", "differentiable", "fused")


def _check_group(group: dict) -> None:
    for name in _UNSUPPORTED:
        if group.get(name):
            raise ValueError(f"quantizedsae_amd.optim.Adam does not support {name} (got {name}={group[name]!r})")
    lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
    if isinstance(lr, torch.Tensor):
        raise ValueError("quantizedsae_amd.optim.Adam takes lr as a Python float (a tensor lr belongs to capturable)")
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0:
        raise ValueError(f"Invalid betas: {(b1, b2)}")
    clip, decay = group.get("max_grad_norm"), group.get("ema_decay")
    if clip is not None and (isinstance(clip, bool) or not isinstance(clip, (int, float)) or not 0.0 < clip < math.inf):
        raise ValueError(f"Invalid max_grad_norm: {clip!r} (expected None or a finite number > 0)")
    if decay is not None and (isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay < 1.0):
        raise ValueError(f"Invalid ema_decay: {decay!r} (expected None or a float in [0, 1))")


class Adam(torch.optim.Optimizer):
    """Adam (no weight decay, amsgrad or maximize) with the step in HIP.

    ``model``: the SAE whose parameters these are.  For a top-k model the encoder pair takes the fused route in every step
    in which encoder weight and bias are both in this optimizer with the same lr / betas / eps and step count, both have
    a gradient, and the weight is 16-byte aligned; in any other step, and for any other model class, every parameter
    goes through the plain kernel and the model's caches notice the new version counters by themselves.

    The keyword-only options after ``model`` are torch.optim.Adam's and exist so that the param groups carry torch's keys
    (state dicts load both ways): a truthy ``weight_decay``, ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``
    or ``fused`` is a ``ValueError`` that names it (``fused`` also because torch reads it from a loaded state dict to place
    ``step`` on the device); ``foreach`` has no meaning here -- there is one implementation -- and is kept as given.

    ``max_grad_norm``: clip the joint L2 norm of all gradients of a step to this value (a finite number > 0), as
    ``torch.nn.utils.clip_grad_norm_`` would.  One number for the whole optimizer: a differing value in any param group is a
    ``ValueError``.  ``step()`` makes one ``grad_norm`` call over every parameter that has a gradient, in param-group order,
    and every step kernel of that step reads the same coefficient word.  ``.grad`` IS LEFT UNSCALED -- what reads it after
    the step (``ModelWatch``, a logger) sees the raw gradients.  ``last_clip`` is the device report of the last step,
    ``clip_report()`` its host copy.
    ``ema_decay``: a float in [0, 1); ``state[p]["ema"]`` starts as a copy of ``p`` at the parameter's first step and moves
    towards the new ``p`` by ``1 - ema_decay`` in the step kernel.  ``ema_state`` (a dict parameter -> tensor): where the
    averages live instead, so that a caller that builds a fresh optimizer per epoch keeps them (``state[p]["ema"]`` is then
    the same tensor; the dict wins over a loaded state dict).  ``ema_weights()`` exchanges weights and averages for the
    duration of a block.
    Both options are param-group keys next to torch's, present only when set; a state dict that carries them (and the
    per-parameter ``"ema"``) loads into ``torch.optim.Adam``, which then steps without them.
    The fused encoder route additionally needs weight and bias to agree on ``ema_decay``."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, *, model: Optional[torch.nn.Module] = None,
                 weight_decay: float = 0, amsgrad: bool = False, maximize: bool = False, foreach: Optional[bool] = None,
                 capturable: bool = False, differentiable: bool = False, fused: Optional[bool] = None,
                 max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None, ema_state: Optional[dict] = None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=False)
        self._recipe = {}                                  # the recipe's keys that are set: group keys only then
        if max_grad_norm is not None:
            self._recipe["max_grad_norm"] = max_grad_norm
        if ema_decay is not None:
            self._recipe["ema_decay"] = ema_decay
        defaults.update(self._recipe)
        _check_group(defaults)
        if ema_state is not None and not isinstance(ema_state, dict):
            raise ValueError(f"ema_state must be a dict parameter -> tensor, got {type(ema_state).__name__}")
        if ema_state is not None and ema_decay is None:
            raise ValueError("ema_state needs ema_decay")
        self._model = model if isinstance(model, TopKCore) else None
        self._owner = model                                # whose caches ema_weights() invalidates
        self._ema_state = ema_state
        self._coef = None                                  # the coefficient word of the last clipped step
        #: the device report of the last clipped step (``ops.grad_norm``), or None
        self.last_clip = None
        super().__init__(params, defaults)

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        for group in self.param_groups:                    # a dict saved without the recipe's keys leaves this optimizer's
            for key, value in self._recipe.items():
                group.setdefault(key, value)

    def add_param_group(self, param_group: dict) -> None:
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            _check_group(group)
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise ValueError(f"quantizedsae_amd.optim.Adam steps fp32 parameters (got {p.dtype})")
                if not p.is_contiguous():
                    raise ValueError("quantizedsae_amd.optim.Adam steps contiguous parameters "
                                     f"(got shape {tuple(p.shape)}, strides {p.stride()})")
        except ValueError:
            self.param_groups.pop()
            raise

    def _state_of(self, p):
        state = self.state[p]
        if len(state) == 0:
            # a host scalar, fp32 (fp64 under a float64 default dtype): where torch's non-capturable Adam keeps it
            state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64
                                         else torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    @staticmethod
    def _scalars(group, t: float):
        """The six scalars of step t in Python floats, as torch's single-tensor Adam computes them."""
        lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
        return (1 - b1, b2, 1 - b2, math.sqrt(1 - b2 ** t), eps, lr / (1 - b1 ** t))

    def _encoder_pair(self, todo):
        """-> (weight, bias) when this step's encoder pair qualifies for the fused route, else None.  ``todo`` maps a
        parameter with a gradient to its group."""
        if self._model is None:
            return None
        lin = self._model.encoder.linear
        W, b = lin.weight, getattr(lin, "bias", None)
        if b is None or W not in todo or b not in todo:
            return None
        gW, gb = todo[W], todo[b]
        if (gW["lr"], tuple(gW["betas"]), gW["eps"], gW.get("ema_decay")) != \
                (gb["lr"], tuple(gb["betas"]), gb["eps"], gb.get("ema_decay")):
            return None
        sW, sb = self.state.get(W), self.state.get(b)
        tW = float(sW["step"]) if sW else 0.0
        tb = float(sb["step"]) if sb else 0.0
        if tW != tb or W.dim() != 2 or W.data_ptr() % 16 != 0 or tuple(b.shape) != (W.shape[0],):
            return None
        return W, b

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        todo = {}
        for group in self.param_groups:
            _check_group(group)                        # a loaded state dict may have brought other options
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("quantizedsae_amd.optim.Adam does not support sparse gradients")
                if not p.is_cuda:
                    raise RuntimeError(f"quantizedsae_amd.optim.Adam runs on MI355X only; a parameter is on {p.device} "
                                       "(no CPU fallback exists)")
                todo[p] = group
        clips = {group.get("max_grad_norm") for group in self.param_groups}
        if len(clips) > 1:
            raise ValueError(f"quantizedsae_amd.optim.Adam: max_grad_norm is one number for the whole optimizer, the param "
                             f"groups hold {sorted(clips, key=repr)}")
        clip = clips.pop() if clips else None
        grads = {p: (p.grad if p.grad.is_contiguous() else p.grad.contiguous()) for p in todo}
        coef = None
        if clip is not None and todo:
            T = len(todo)
            keep = self.last_clip is not None and self.last_clip.shape[0] == ops.GRAD_NORM_HEAD + T \
                and self.last_clip.device == next(iter(todo)).device
            coef, self.last_clip = ops.grad_norm(list(grads.values()), clip, self._coef if keep else None,
                                                 self.last_clip if keep else None)
            self._coef = coef
        pair = self._encoder_pair(todo)
        for p, group in todo.items():
            if pair is not None and p is pair[1]:
                continue                               # the bias goes with its weight
            state = self._state_of(p)
            state["step"] += 1
            scalars = self._scalars(group, float(state["step"]))
            decay = group.get("ema_decay")
            ema = self._ema_of(p, state) if decay is not None else None
            if pair is not None and p is pair[0]:
                self._step_pair(pair[1], grads[p], grads[pair[1]], state, scalars, coef, ema, decay)
            elif coef is None and ema is None:
                ops.adam_step(p.detach(), grads[p], state["exp_avg"], state["exp_avg_sq"], *scalars)
            else:
                ops.adam_step_clipped(p.detach(), grads[p], state["exp_avg"], state["exp_avg_sq"], *scalars, coef=coef, ema=ema,
                                      one_minus_decay=0.0 if decay is None else 1 - decay)
        return loss

    def _ema_of(self, p, state):
        """The average of p: a copy of p at the parameter's first step; kept in ``ema_state`` where one was given."""
        if self._ema_state is not None:
            ema = self._ema_state.get(p)
            if ema is None:
                ema = self._ema_state[p] = p.detach().clone(memory_format=torch.contiguous_format)
            state["ema"] = ema
        elif "ema" not in state:
            state["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
        return state["ema"]

    def clip_report(self) -> Optional[ClipReport]:
        """The report of the last clipped step on the host (one copy of 32 + 8 T bytes), or None before the first."""
        if self.last_clip is None:
            return None
        words = self.last_clip.cpu()
        f = words.view(torch.float64)
        return ClipReport(norm=f[1].item(), coef=f[2].item(), clipped=bool(words[3].item()),
                          per_tensor=tuple(f[ops.GRAD_NORM_HEAD:].tolist()))

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block every parameter that has an average holds it, and the average holds the weights; on exit they
        are exchanged back.  Plain torch copies under ``no_grad`` (version counters move, every cache keyed on a parameter
        rebuilds by itself; a model with ``invalidate_packed`` is told as well).  Not for the hot path."""
        def exchange():
            with torch.no_grad():
                for group in self.param_groups:
                    for p in group["params"]:
                        ema = self._ema_state.get(p) if self._ema_state is not None else self.state.get(p, {}).get("ema")
                        if ema is not None:
                            kept = p.detach().clone()
                            p.copy_(ema)
                            ema.copy_(kept)
            if hasattr(self._owner, "invalidate_packed"):
                self._owner.invalidate_packed()
        exchange()
        try:
            yield self
        finally:
            exchange()

    def _step_pair(self, b, gW, gb, stateW, scalars, coef, emaW, decay) -> None:
        model = self._model
        lin = model.encoder.linear
        W = lin.weight
        stateb = self._state_of(b)
        stateb["step"] += 1
        emab = self._ema_of(b, stateb) if decay is not None else None
        # the buffers of the copy that is about to go stale take the new one (work on one stream is ordered)
        Wq = meta = None
        old = model._pref_cache.peek()
        if isinstance(old, dict) and isinstance(old.get("Wq"), torch.Tensor) and isinstance(old.get("meta"), torch.Tensor):
            oq, om = old["Wq"], old["meta"]
            if oq.shape == W.shape and oq.dtype == torch.float16 and oq.device == W.device and oq.is_contiguous() \
                    and oq.data_ptr() % 16 == 0 and tuple(om.shape) == (4,) and om.dtype == torch.float32 \
                    and om.device == W.device:
                Wq, meta = oq, om
        if coef is None and emaW is None:
            Wq, meta = ops.adam_step_prefilter(W.detach(), gW, stateW["exp_avg"], stateW["exp_avg_sq"], b.detach(), gb,
                                               stateb["exp_avg"], stateb["exp_avg_sq"], *scalars, Wq=Wq, meta=meta)
        else:
            Wq, meta = ops.adam_step_prefilter_clipped(W.detach(), gW, stateW["exp_avg"], stateW["exp_avg_sq"], b.detach(), gb,
                                                       stateb["exp_avg"], stateb["exp_avg_sq"], *scalars, coef=coef, emaW=emaW,
                                                       emab=emab, one_minus_decay=0.0 if decay is None else 1 - decay,
                                                       Wq=Wq, meta=meta)
        # after the op: its writes have moved the version counters that the cache key reads
        model._pref_cache.put((lin.weight, lin.bias), {"Wq": Wq, "meta": meta})
