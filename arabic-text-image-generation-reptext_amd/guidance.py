"""What a true-CFG call may add to the rule ``neg + s·(pos − neg)`` at every step: a guidance interval and projected guidance (APG:
Sadat et al., "Eliminating oversaturation and artifacts of high guidance scales"; diffusers ships it as a guider — the rule is
recalled, parity with diffusers is unpinned). Host only. The setting is a plain attribute of a pipeline, ``pipe.guider`` (None by
default), read by ``_generate`` when true CFG is on for the call; DESIGN.md §7.

A guided step, per sample and in fp32, with p the positive and u the negative half of the model output over the sample's elements:

    d = (p − u) + β·r_prev              r_prev: the d of the guided step before; β = 0 on the first guided step of a run
    a = Σ d²,  b = Σ d·p,  c = Σ p²
    k = τ > 0 and a > τ² ? τ/√a : 1     the norm clamp
    α = c > 0 ? k·b/c : 0               coefficient of the component of k·d parallel to p
    v = p + (s − 1)·(k·d + (η − 1)·α·p) = p + (s − 1)·(d_orth + η·d_par)

(rt_guidance_reduce_f32 + rt_projected_step_f32, csrc/norm_elem.hip). Outside the interval the step is the plain step on p, with the
models evaluated on the positive half alone."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch


@dataclass(frozen=True)
class TrueCFGGuider:
    start: float = 0.0           # guidance interval, as fractions of the steps that run
    stop: float = 1.0
    eta: float = 1.0             # weight of the component of the difference parallel to the positive prediction
    norm_threshold: float = 0.0  # > 0: the difference's per-sample L2 norm is clamped to it
    momentum: float = 0.0        # beta of the running difference; APG's usual value is negative (-0.5)

    def __post_init__(self):
        for name in ("start", "stop", "eta", "norm_threshold", "momentum"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"TrueCFGGuider: {name} = {v!r} is not a finite number")
        if not (0.0 <= self.start <= 1.0 and 0.0 <= self.stop <= 1.0):
            raise ValueError(f"TrueCFGGuider: the interval ({self.start}, {self.stop}) must lie inside [0, 1]")
        if self.start > self.stop:
            raise ValueError(f"TrueCFGGuider: start {self.start} is above stop {self.stop}")
        if self.norm_threshold < 0:
            raise ValueError(f"TrueCFGGuider: norm_threshold {self.norm_threshold} is negative")
        if abs(self.momentum) >= 1:
            raise ValueError(f"TrueCFGGuider: |momentum| = {abs(self.momentum)} must be below 1")

    @property
    def projected(self) -> bool:
        """The step needs the per-sample sums: anything but the plain mix."""
        return self.eta != 1 or self.norm_threshold > 0 or self.momentum != 0

    @property
    def whole(self) -> bool:
        """The interval covers every step."""
        return self.start == 0 and self.stop == 1


def guided_steps(n: int, guider: TrueCFGGuider) -> Tuple[int, ...]:
    """The steps, of the ``n`` that run, inside the guider's interval: the rule of ``pipeline.union_active_steps``."""
    from .pipeline import union_active_steps

    return union_active_steps(n, float(guider.start), float(guider.stop))


@dataclass(frozen=True)
class Guidance:
    """``LoopExtras.guidance``: the guider of a call that it changes, and the steps it guides."""
    guider: TrueCFGGuider
    steps: Tuple[int, ...]

    def signature(self) -> tuple:            # of a captured loop: host scalars only; its buffers are allocated inside the capture
        return (("guidance", self.steps) + tuple(float(getattr(self.guider, n)) for n in ("eta", "norm_threshold", "momentum")),)


@dataclass
class ProjectedStep:
    """What ``scheduler.step_master_(projected=)`` takes: the guider's three numbers, the two buffers the caller owns (``diff``: fp32, the
    state's shape, the guidance difference of the guided step before; ``partials``: fp32, ``ops.guidance_partials_shape``) and whether
    this is the first guided step of a run (``diff`` is then written and not read)."""
    eta: float
    norm_threshold: float
    momentum: float
    diff: torch.Tensor
    partials: torch.Tensor
    first: bool = True


def loop_guidance(guider: Optional[TrueCFGGuider], cfg: bool, n: int) -> Optional[Guidance]:
    """The record ``_generate`` puts into ``LoopExtras``: None unless true CFG is on and the guider changes the call."""
    if guider is None or not cfg:
        return None
    if not isinstance(guider, TrueCFGGuider):
        raise ValueError(f"pipe.guider must be a TrueCFGGuider or None, not {type(guider).__name__}")
    if not guider.projected and guider.whole:
        return None
    return Guidance(guider, guided_steps(n, guider))
