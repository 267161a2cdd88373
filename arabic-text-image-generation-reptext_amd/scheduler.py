"""FlowMatchEulerDiscreteScheduler with dynamic (exponential) time shifting — the scheduler the reference takes from
diffusers (PIPE:18) and drives at PIPE:948-967 (``set_timesteps(sigmas=..., mu=...)``) and PIPE:1109 (``step``).

Math per SURVEY.md Appendix A.6. The sigma schedule is host-side fp32 (n+1 scalars); ``step`` is one HIP axpy
(fp32 arithmetic, result rounded once to the sample dtype, as diffusers upcasts inside ``step``).

``FlowMatchMultistepScheduler`` is the same grid with a second-order multistep step (Adams–Bashforth 2 in sigma, ``multistep_weights``):
one model evaluation per step as before, plus the velocity of the step before in an fp32 buffer.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Union

import numpy as np
import torch

from . import ops
from .config import Config, flux_scheduler_config


def calculate_shift(image_seq_len, base_seq_len: int = 256, max_seq_len: int = 4096, base_shift: float = 0.5,
                    max_shift: float = 1.16):
    """Linear map seq_len -> mu (PIPE:78-88; note the 1.16 default that the pipeline overrides with config 1.15)."""
    slope = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    return image_seq_len * slope + (base_shift - slope * base_seq_len)


# stochastic sampling: diffusers' switch and this package's eta, with their defaults; a config holds a key only where its value is
# not the default, so a scheduler without the switch saves the file it always saved
STOCHASTIC_DEFAULTS = {"stochastic_sampling": False, "stochastic_eta": 1.0}


@dataclass(frozen=True)
class StochasticStep:
    """What ``step_master_(stochastic=)`` takes: ``rng`` int64 [B, 2] on the state's device, (seed, subsequence) per sample
    (``pipeline.stochastic_rng``), and the two eta scalars (``FlowMatchEulerDiscreteScheduler.stochastic_step`` forms them)."""
    rng: torch.Tensor
    eta: float
    sqrt_1m_eta2: float


class FlowMatchEulerDiscreteScheduler:
    order = 1

    def __init__(self, **config):
        stochastic = {k: config.pop(k, default) for k, default in STOCHASTIC_DEFAULTS.items()}
        if not isinstance(stochastic["stochastic_sampling"], bool):
            raise ValueError(f"stochastic_sampling must be a bool, got {stochastic['stochastic_sampling']!r}")
        eta = stochastic["stochastic_eta"] = float(stochastic["stochastic_eta"])
        if not 0.0 < eta <= 1.0:          # 0 is the Euler step, reached in the limit only: it draws nothing and is this scheduler without the switch
            raise ValueError(f"stochastic_eta must lie in (0, 1], got {eta}")
        self.config = flux_scheduler_config(**config)
        self.config.update({k: v for k, v in stochastic.items() if v != STOCHASTIC_DEFAULTS[k]})
        self.timesteps: Optional[torch.Tensor] = None
        self.sigmas: Optional[torch.Tensor] = None      # host fp32, n+1 entries (trailing 0)
        self._step_index: Optional[int] = None
        self._begin_index: Optional[int] = None
        self.num_inference_steps: Optional[int] = None

    @classmethod
    def from_config(cls, config):
        return cls(**{k: v for k, v in dict(config).items() if not k.startswith("_")})

    @property
    def step_index(self):
        return self._step_index

    @property
    def stochastic_sampling(self) -> bool:
        return bool(self.config.get("stochastic_sampling", False))

    @property
    def stochastic_eta(self) -> float:
        return float(self.config.get("stochastic_eta", 1.0))

    def stochastic_step(self, rng: torch.Tensor) -> StochasticStep:
        """The ``stochastic=`` record of this scheduler's eta for a call's ``rng``; sqrt(1 − eta²) in double."""
        eta = self.stochastic_eta
        return StochasticStep(rng, eta, math.sqrt(max(0.0, 1.0 - eta * eta)))

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def _time_shift(self, mu: float, s: np.ndarray) -> np.ndarray:
        return math.exp(mu) / (math.exp(mu) + (1.0 / s - 1.0))

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, sigmas: Optional[List[float]] = None,
                      mu: Optional[float] = None, timesteps: Optional[List[float]] = None):
        cfg = self.config
        if cfg.use_dynamic_shifting and mu is None:
            raise ValueError("`mu` must be passed when `use_dynamic_shifting` is set to be `True`")
        if sigmas is None:
            if timesteps is not None:
                s = np.asarray(timesteps, dtype=np.float32) / cfg.num_train_timesteps
            else:
                if num_inference_steps is None:
                    raise ValueError("pass num_inference_steps, sigmas or timesteps")
                # diffusers takes the grid's end points from the sigma table its constructor built — which, without dynamic
                # shifting, has ALREADY been passed through the static shift (sigma_max stays 1, sigma_min becomes
                # shift·s/(1+(shift-1)·s) at s = 1/num_train_timesteps) — and then applies the shift to the grid once more below.
                # Restated from knowledge of diffusers 0.36 (parity unpinned: the package is absent); FLUX.1's scheduler config
                # sets use_dynamic_shifting=True and never takes this branch.
                smax, smin = 1.0, 1.0 / cfg.num_train_timesteps
                if not cfg.use_dynamic_shifting:
                    smin = cfg.shift * smin / (1 + (cfg.shift - 1) * smin)
                t = np.linspace(smax * cfg.num_train_timesteps, smin * cfg.num_train_timesteps, num_inference_steps)
                s = (t / cfg.num_train_timesteps).astype(np.float32)
        else:
            s = np.asarray(sigmas, dtype=np.float32)
        if cfg.use_dynamic_shifting:
            s = self._time_shift(float(mu), s.astype(np.float32)).astype(np.float32)
        else:
            s = (cfg.shift * s / (1 + (cfg.shift - 1) * s)).astype(np.float32)
        self.num_inference_steps = len(s)
        sig = torch.from_numpy(np.ascontiguousarray(s)).to(torch.float32)
        self.timesteps = (sig * cfg.num_train_timesteps).to(device=device)
        self.sigmas = torch.cat([sig, torch.zeros(1)])
        self._step_index = None
        self._begin_index = None

    def _init_step_index(self, timestep):
        if self._begin_index is not None:
            self._step_index = self._begin_index
            return
        t = float(timestep)
        idx = (self.timesteps.cpu() == t).nonzero()
        self._step_index = int(idx[1 if len(idx) > 1 else 0]) if len(idx) > 0 else 0

    def _advance(self):
        """(sigmas[i], sigmas[i + 1]) of the step about to be taken, and the index moves on. The loop walks the timesteps in order, so
        the first step is the begin index or 0: looking the timestep up would cost a device sync."""
        if self._step_index is None:
            self._step_index = self._begin_index if self._begin_index is not None else 0
        i = self._step_index
        self._step_index = i + 1
        return self.sigmas[i], self.sigmas[i + 1]

    def _advance_weight(self):
        """``_advance`` plus the multistep weight of the step about to be taken: 0, the Euler rule."""
        return (*self._advance(), 0.0)

    def _history(self, history: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """The history the step uses: the Euler rule has none (returns None) and refuses one."""
        if history is not None:
            raise TypeError("step_master_: history= belongs to the multistep scheduler, the Euler scheduler keeps no velocity")

    def step_master_(self, v: torch.Tensor, sample32: torch.Tensor, sample_bf16: Optional[torch.Tensor] = None, *,
                     v_text: Optional[torch.Tensor] = None, s: Optional[float] = None, repaint=None,
                     history: Optional[torch.Tensor] = None, projected=None, stochastic: Optional[StochasticStep] = None) -> None:
        """In-place step on an fp32 master copy of the latents (used by this repo's pipelines between steps; ``step`` keeps
        the diffusers contract of returning the model dtype), one kernel. Advances the step index exactly like ``step``.
        ``v_text``: true CFG, the velocity is ``v + s·(v_text − v)`` (``v`` the unconditional half), mixed in fp32 inside the kernel and
        not rounded to bf16 before the state takes it. ``repaint`` (a record with ``src32``, ``noise32``, ``mask``): where ``mask`` is 0
        the state becomes the source re-noised to the NEXT sigma, ``scale_noise(src32, sigmas[i + 1], noise32)`` — the source itself
        after the last step. ``projected`` (a ``guidance.ProjectedStep``; needs ``v_text`` and ``s``): projected guidance in the mix's
        place, two kernels; its ``diff`` receives this step's guidance difference and is read unless ``projected.first`` (no momentum
        on the first guided step of a run); ``s − 1`` is formed from the scale in double inside the op. ``history`` (the multistep
        scheduler's; fp32, the state's shape) is read unless it is empty — it may then be uninitialised memory — and receives this
        step's velocity, under true CFG the mixed or projected one in fp32; the blend of a repaint comes after. ``stochastic`` (a
        ``StochasticStep``; a scheduler with ``stochastic_sampling`` needs it, any other takes the rule from it all the same): the
        predicted clean image ``x − σ·v`` re-noised to the next sigma in the Euler rule's place, with fresh noise drawn inside the kernel
        from (``rng``, the absolute step index); after the last step it is the clean image itself. ``sample32``'s leading dimension is
        then the batch."""
        history = self._history(history)
        if stochastic is None and self.stochastic_sampling:
            raise ValueError("step_master_: a scheduler with stochastic_sampling needs stochastic= (scheduler.stochastic_step(rng))")
        if stochastic is not None and history is not None:
            raise ValueError("step_master_: stochastic= and history= exclude each other (stochastic sampling is first order)")
        sigma, sigma_next, w = self._advance_weight()
        rp = {} if repaint is None else dict(sigma_next=float(sigma_next), src32=repaint.src32, noise32=repaint.noise32, mask=repaint.mask)
        if stochastic is not None:
            rp = dict(rp, sigma_next=float(sigma_next), stochastic=ops.StochasticArgs(
                stochastic.rng, float(sigma), stochastic.eta, stochastic.sqrt_1m_eta2, self._step_index - 1))
        if projected is None:
            ops._master_step_f32("step_master_", sample32, v.contiguous(), None if v_text is None else v_text.contiguous(), float(s or 0.0),
                                 float(sigma_next - sigma), sample_bf16, hist=history, w=w, **rp)
        elif v_text is None or s is None:
            raise ValueError("step_master_: projected= needs v_text= and s= (true CFG)")
        else:
            ops.projected_step_f32_(sample32, v.contiguous(), v_text.contiguous(), projected.diff, projected.partials, float(s),
                                    float(projected.eta), float(projected.norm_threshold), 0.0 if projected.first else float(projected.momentum),
                                    float(sigma_next - sigma), sample_bf16, hist32=history, w=float(w), **rp)

    def scale_noise(self, sample: torch.Tensor, sigma_or_timestep, noise: torch.Tensor) -> torch.Tensor:
        """``sigma·noise + (1 − sigma)·sample``: the forward process of flow matching (diffusers' rule, recalled). A value of at most 1 is
        the sigma itself; a larger one is a timestep of the current schedule, whose sigma is looked up (t / num_train_timesteps where it
        is not on the schedule). Computed in ``sample``'s dtype, each product and the sum rounded once."""
        t = float(sigma_or_timestep)
        if t <= 1.0:
            sigma = t
        else:
            idx = (self.timesteps.cpu() == t).nonzero() if self.timesteps is not None else []
            sigma = float(self.sigmas[int(idx[0])]) if len(idx) > 0 else t / self.config.num_train_timesteps
        return sigma * noise + (1.0 - sigma) * sample

    def step(self, model_output: torch.Tensor, timestep: Union[float, torch.Tensor], sample: torch.Tensor,
             return_dict: bool = True, generator=None, **unused):
        """The diffusers contract: the sample comes and goes in the model dtype. With ``stochastic_sampling`` the step is the op of
        ``step_master_`` on an fp32 temporary, and ``generator`` (one, a list per sample, or None: ``pipeline.stochastic_rng``) names the
        noise streams; the sample's leading dimension is the batch."""
        if self.stochastic_sampling:
            from .pipeline import stochastic_rng

            sigma, sigma_next = self._advance()
            x32 = sample.to(torch.float32).contiguous().clone()
            if x32.dim() < 2:
                x32 = x32[None]
            st = self.stochastic_step(stochastic_rng(generator, x32.shape[0]).to(x32.device))
            ops.stochastic_step_f32_(x32, model_output.contiguous().view(x32.shape), ops.StochasticArgs(
                st.rng, float(sigma), st.eta, st.sqrt_1m_eta2, self._step_index - 1), float(sigma_next))
            prev = x32.view(sample.shape).to(model_output.dtype)
            return (prev,) if not return_dict else Config(prev_sample=prev)
        sigma, sigma_next = self._advance()
        prev = sample.to(model_output.dtype).clone()
        ops.euler_step_(prev, model_output.contiguous(), float(sigma_next - sigma))
        if not return_dict:
            return (prev,)
        return Config(prev_sample=prev)


def _multistep_weight(sigmas, i: int) -> float:
    """w_i = (σ_{i+1} − σ_i) / (2·(σ_i − σ_{i−1})) in float64 from the fp32 table."""
    a, b, c = float(sigmas[i - 1]), float(sigmas[i]), float(sigmas[i + 1])
    return (c - b) / (2.0 * (b - a))


def multistep_weights(sigmas, begin: int = 0, order: int = 2) -> List[float]:
    """The weight of every step of the second-order multistep rule (Adams–Bashforth 2 on the sigma grid)

        x_{i+1} = x_i + dσ_i·(v_i + w_i·(v_i − v_{i−1})),   dσ_i = σ_{i+1} − σ_i,   w_i = dσ_i / (2·dσ_{i−1})

    for a run that starts at step ``begin``: that step has no velocity before it and is first order, w = 0 (as are the entries before
    it, which do not run). ``sigmas``: the n + 1 entries of the scheduler's table; n weights come back, computed in float64 from the
    table's values. ``order`` 1: all zero, the Euler rule."""
    if order not in (1, 2):
        raise ValueError(f"multistep_weights: order {order} is not supported (1 or 2)")
    n = len(sigmas) - 1
    return [0.0 if order == 1 or i <= begin else _multistep_weight(sigmas, i) for i in range(n)]


class FlowMatchMultistepScheduler(FlowMatchEulerDiscreteScheduler):
    """The Euler scheduler's grid with a second-order multistep step (``multistep_weights``): one model evaluation per step, as for
    Euler, plus the velocity of the step before. That velocity lives in an fp32 ``history`` tensor of the state's shape which the
    CALLER of ``step_master_`` owns (the denoising loop allocates it beside its fp32 state; a captured loop keeps it in the graph's
    pool); the scheduler holds host state only: whether the history holds a velocity. ``set_timesteps``, ``set_begin_index`` and
    ``reset_history`` empty it, and the step after is first order. ``solver_order=1`` is the Euler scheduler."""
    order = 1               # model evaluations per step (the pipelines' progress and warm-up arithmetic), not the solver's order

    def __init__(self, **config):
        solver_order = int(config.pop("solver_order", 2))
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order {solver_order} is not supported (1 or 2)")
        super().__init__(**config)
        if solver_order > 1 and self.stochastic_sampling:
            raise ValueError("stochastic_sampling needs solver_order=1: the velocity of the step before belongs to a state that the "
                             "fresh noise has replaced, it is no history of the same trajectory")
        self.config["solver_order"] = solver_order
        self._history_len = 0                       # velocities the history holds: 0 or 1
        self._step_history: Optional[torch.Tensor] = None       # the history of ``step`` (the diffusers contract), fp32

    @classmethod
    def from_config(cls, config):
        """From a saved config of this class or of the Euler class; keys of other schedulers are ignored, as the loader ignores them."""
        known = set(flux_scheduler_config().keys()) | {"solver_order"} | set(STOCHASTIC_DEFAULTS)
        return cls(**{k: v for k, v in dict(config).items() if k in known})

    @property
    def solver_order(self) -> int:
        return self.config["solver_order"]

    def reset_history(self) -> None:
        """Forget the velocity of the step before: the next step is first order."""
        self._history_len = 0
        self._step_history = None

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, sigmas: Optional[List[float]] = None,
                      mu: Optional[float] = None, timesteps: Optional[List[float]] = None):
        """The Euler scheduler's grid, unchanged (the signature is spelled out: ``retrieve_timesteps`` inspects it); empties the history."""
        super().set_timesteps(num_inference_steps, device=device, sigmas=sigmas, mu=mu, timesteps=timesteps)
        self.reset_history()

    def set_begin_index(self, begin_index: int = 0):
        super().set_begin_index(begin_index)
        self.reset_history()

    def _advance_weight(self):
        """``_advance`` plus the weight of the step about to be taken; at order 2 the history then counts as holding its velocity."""
        if self.solver_order == 1:
            return super()._advance_weight()
        sigma, sigma_next = self._advance()
        i = self._step_index - 1
        w = _multistep_weight(self.sigmas, i) if self._history_len > 0 and i > 0 else 0.0
        self._history_len = 1
        return sigma, sigma_next, w

    def _history(self, history: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """Order 2 needs the caller's history; order 1 is the Euler rule and leaves one unused."""
        if self.solver_order > 1 and history is None:
            raise ValueError("step_master_: the multistep scheduler needs history=, an fp32 tensor of the state's shape")
        return history if self.solver_order > 1 else None

    def step(self, model_output: torch.Tensor, timestep: Union[float, torch.Tensor], sample: torch.Tensor,
             return_dict: bool = True, **unused):
        if self.solver_order == 1:
            return super().step(model_output, timestep, sample, return_dict=return_dict, **unused)
        hist = self._step_history if self._history_len > 0 else None
        if hist is None or hist.shape != sample.shape or hist.device != sample.device:
            self._history_len = 0
            hist = torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
        sigma, sigma_next, w = self._advance_weight()
        x32 = sample.to(torch.float32).contiguous().clone()
        ops.multistep_step_f32_(x32, model_output.contiguous(), hist, w, float(sigma_next - sigma))
        self._step_history = hist
        prev = x32.to(model_output.dtype)
        if not return_dict:
            return (prev,)
        return Config(prev_sample=prev)
