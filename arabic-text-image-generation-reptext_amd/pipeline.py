"""FluxControlNetPipeline (text-to-image with RepText glyph conditions) on the MI355X kernels.

Interface parity target: /root/reference/RepText/pipeline_flux_controlnet.py
  * constructor components ........................ PIPE:194-226
  * __call__ keyword names / defaults / returns ... PIPE:751-781, 1132-1148
  * check_inputs errors ........................... PIPE:485-531
  * helper statics (ids, pack, unpack) ............ PIPE:533-570
  * latent / hint preparation ..................... PIPE:573-731
  * denoising loop semantics (quirks Q1-Q5) ....... PIPE:1016-1130, SURVEY.md §8a
The control flow is organised as plan -> prepare -> denoise -> decode stages over device-resident state; the
per-step work is a fixed sequence of HIP launches (mmdit.py) with the regional mask and the sum over text lines fused
into the ControlNet's zero-linear epilogues.
"""
from __future__ import annotations

import contextlib
import functools
import inspect
import json
import math
import os
from dataclasses import dataclass, fields, make_dataclass, replace
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .controlnet import FluxControlNetModel, FluxMultiControlNetModel, active_row_window
from .image_processor import PipelineImageInput, VaeImageProcessor
from .guidance import Guidance, ProjectedStep, loop_guidance
from .scheduler import STOCHASTIC_DEFAULTS, FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler, calculate_shift
from .transformer import FluxTransformer2DModel
from .utils import randn_tensor
from .vae import AutoencoderKL


@dataclass
class FluxPipelineOutput:
    images: Any


def retrieve_latents(encoder_output, generator: Optional[torch.Generator] = None, sample_mode: str = "sample"):
    """PIPE:91-101."""
    if hasattr(encoder_output, "latent_dist") and sample_mode == "sample":
        return encoder_output.latent_dist.sample(generator)
    if hasattr(encoder_output, "latent_dist") and sample_mode == "argmax":
        return encoder_output.latent_dist.mode()
    if hasattr(encoder_output, "latents"):
        return encoder_output.latents
    raise AttributeError("Could not access latents of provided encoder_output")


def retrieve_timesteps(scheduler, num_inference_steps: Optional[int] = None, device=None, timesteps: Optional[List[int]] = None,
                       sigmas: Optional[List[float]] = None, **kwargs):
    """PIPE:104-160: drive ``scheduler.set_timesteps`` with a step count, custom timesteps or custom sigmas."""
    if timesteps is not None and sigmas is not None:
        raise ValueError("Only one of `timesteps` or `sigmas` can be passed. Please choose one to set custom values")
    accepted = set(inspect.signature(scheduler.set_timesteps).parameters.keys())
    if timesteps is not None:
        if "timesteps" not in accepted:
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" timestep schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kwargs)
    elif sigmas is not None:
        if "sigmas" not in accepted:
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" sigmas schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(sigmas=sigmas, device=device, **kwargs)
    else:
        scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
    return scheduler.timesteps, len(scheduler.timesteps)


class _Progress:
    def __init__(self, total, disable=False):
        self.bar = None
        if not disable:
            try:
                from tqdm.auto import tqdm

                self.bar = tqdm(total=total)
            except Exception:
                self.bar = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.bar is not None:
            self.bar.close()

    def update(self, n=1):
        if self.bar is not None:
            self.bar.update(n)


# The ControlNet tower runs on a side stream next to the transformer (see _denoise_eager): within a step the two chains are
# independent except that transformer block i reads tower sample i // 4. Bitwise neutral (test_tower_stream_overlap_is_bitwise_
# neutral). Measured on MI355X: -0.5 % per image with the eager loop, -1.1 % when the loop is replayed from its hipGraph (2.105-2.110
# vs 2.125-2.137 s, alternating runs on one box: the fork/join is then part of the graph instead of host-side event calls). On by
# default (RT_OVERLAP_TOWER=0 turns it off); bench.py's roofline pass and the rocprof summaries run with it off so that every kernel
# is alone on the chip when it is timed.
OVERLAP_TOWER = os.environ.get("RT_OVERLAP_TOWER", "1") == "1"
# RT_GRAPH=1 (default): the denoising loop of a call signature seen before is captured ONCE into a hipGraph (every kernel of the
# 28 steps, ~7 000 nodes, host scalars baked in) and replayed for later calls with the same signature: bitwise the eager result,
# the host returns after ~5 ms instead of enqueueing ~13 000 launches, the GPU loses the launch bubbles (-0.7 % per image).
# The first call of a signature always runs eagerly (it also warms every lazily built buffer); capture failures fall back to
# eager for good. `pipe.capture_graphs = False` (or RT_GRAPH=0) turns it off.
GRAPH_CAPTURE = os.environ.get("RT_GRAPH", "1") == "1"
# A regional mask is zero outside the box of its text line, and a zero row of a tower sample adds exactly ±0 to the transformer. With
# RT_TOWER_WINDOW=1 (default) the tower's zero-linears compute only the row window that holds every non-zero mask row, and its last
# evaluated block — read by nothing but its zero-linear — runs attention, out, LayerNorm, ff1 and ff2 for those rows alone.
TOWER_WINDOW = os.environ.get("RT_TOWER_WINDOW", "1") == "1"
GRAPH_CACHE_MAX = 2


def union_active_steps(num_steps: int, start: float, end: float) -> Tuple[int, ...]:
    """The steps, of ``num_steps``, at which a tower with the guidance interval [start, end] is evaluated: step i iff
    ``not (i / n < start or (i + 1) / n > end)`` — diffusers' ``controlnet_keep`` (recalled, not read). ``start > end`` gives none."""
    n = int(num_steps)
    return tuple(i for i in range(n) if not (i / n < start or (i + 1) / n > end))


def tower_schedule(num_steps: int, cn_steps: int, n_lines: int, union_active: Optional[Tuple[int, ...]] = None,
                   n_extra: int = 0) -> List[List[Tuple[int, int]]]:
    """The towers of every denoising step in evaluation order — the order of the sum into the sample buffers — from host scalars alone.
    Entry i lists (tower, position in that tower's modulation table) for step i; towers are numbered [the union tower, if
    ``union_active`` names a step] + [text lines] + [extra towers]. The union tower comes first, at its active steps
    (``union_active_steps``), also where no text tower runs; its table holds those steps only, so its position is the step's index among
    them. The text lines follow at steps i < ``cn_steps`` (PIPE:1076-1087; past them no tower runs, Q3), then the extra towers: their
    residuals are added to the text towers' and dropped without them (INP:1231-1245), so they run only where text towers do. Both take
    table position i."""
    union = tuple(union_active or ())
    first_line = 1 if union else 0
    n_text = n_lines + n_extra if n_lines > 0 else 0
    return [([(0, union.index(i))] if i in union else []) + ([(first_line + k, i) for k in range(n_text)] if i < cn_steps else [])
            for i in range(int(num_steps))]


@dataclass
class _Tower:
    """One ControlNet tower of ``_denoise_eager``. ``masked``: a text line, which takes the regional mask (``rowscale``) and the row
    window; the union and extra towers write every row. ``static``: the loop-invariant embeddings of (prompt, ``hint``)."""
    model: FluxControlNetModel
    hint: torch.Tensor
    scale: Any
    rowscale: Optional[torch.Tensor]
    table: Any
    masked: bool
    static: Any = None


# ``pipe._sample_cache``: the tower sample buffers of one shape and the row window outside which ``double`` reads zero (None: no promise)
_SampleCache = make_dataclass("_SampleCache", ["key", "double", "single", ("window", Any, None)])


TRUE_CFG_ARGUMENTS = ("negative_prompt", "negative_prompt_2", "true_cfg_scale", "negative_prompt_embeds", "negative_pooled_prompt_embeds",
                      "negative_ip_adapter_image", "negative_ip_adapter_image_embeds")


@dataclass
class CallExtensions:
    """The keyword-only extensions of a ``__call__``, as the caller passed them: the IP-Adapter's image prompt, the second ControlNet's
    four arguments and the negative prompt's seven (``TRUE_CFG_ARGUMENTS``; diffusers' names, rules recalled: DESIGN.md §7)."""
    ip_adapter_image: Any = None
    ip_adapter_image_embeds: Any = None
    control_image_union: Any = None
    controlnet_conditioning_scale_union: float = 1.0
    control_guidance_start_union: float = 0.0
    control_guidance_end_union: float = 1.0
    negative_prompt: Any = None
    negative_prompt_2: Any = None
    true_cfg_scale: float = 1.0
    negative_prompt_embeds: Any = None
    negative_pooled_prompt_embeds: Any = None
    negative_ip_adapter_image: Any = None
    negative_ip_adapter_image_embeds: Any = None


LINE_PROMPT_ARGUMENTS = ("control_prompt", "control_prompt_embeds", "control_prompt_max_sequence_length")
MAX_LINE_PROMPTS = 30                   # groups: the base prompt, one per line prompt, the image tokens — at most 32 (rt_attention_fwd_grouped)


@dataclass
class LineCallExtensions(CallExtensions):
    """``CallExtensions`` of a call that names a per-line prompt (``LINE_PROMPT_ARGUMENTS``): the record with its three keywords behind
    the thirteen. ``accepts_call_extensions`` builds it only for such a call; every other call carries the plain record it always did."""
    control_prompt: Any = None                          # one entry per text line, parallel to control_image: a string or None
    control_prompt_embeds: Any = None                   # the same as T5 embeddings: one [B, L, joint_attention_dim] tensor or None per line
    control_prompt_max_sequence_length: int = 128       # L: a multiple of 64, at most 512


REGIONAL_IP_ARGUMENTS = ("ip_adapter_mask", "control_ip_adapter_image", "control_ip_adapter_image_embeds", "control_ip_adapter_scale")


@dataclass
class RegionalIPCallExtensions(LineCallExtensions):
    """``LineCallExtensions`` of a call that names a regional image prompt (``REGIONAL_IP_ARGUMENTS``), so that a call may name both
    families. ``accepts_call_extensions`` builds it only for such a call."""
    ip_adapter_mask: Any = None                         # the region of ip_adapter_image[_embeds]: one mask, in a control_mask entry's forms
    control_ip_adapter_image: Any = None                # one entry per text line, parallel to control_image: an image or None
    control_ip_adapter_image_embeds: Any = None         # the same as embeddings: [B,1,E], [B,E] or [1,E], or None, per line
    control_ip_adapter_scale: Any = 1.0                 # a float, or one per text line


ISOLATION_ARGUMENTS = ("control_prompt_isolation",)
MAX_KEY_CLASSES = 32                    # rt_attention_fwd_keyed: a class id selects a bit of a row's 32-bit word


@dataclass
class IsolationCallExtensions(RegionalIPCallExtensions):
    """``RegionalIPCallExtensions`` of a call that names ``control_prompt_isolation`` (``ISOLATION_ARGUMENTS``).
    ``accepts_call_extensions`` builds it only for such a call."""
    control_prompt_isolation: bool = False              # per-line prompts under the per-key rule of ``line_prompt_classes``


LINE_SCALE_ARGUMENTS = ("control_prompt_scale",)
LINE_SCALE_RANGE = (1.0 / 64, 64.0)     # below it a line prompt is as good as hidden, above it the only text its box sees: a stated condition


@dataclass
class LineScaleCallExtensions(IsolationCallExtensions):
    """``IsolationCallExtensions`` of a call that names ``control_prompt_scale`` (``LINE_SCALE_ARGUMENTS``).
    ``accepts_call_extensions`` builds it only for such a call."""
    control_prompt_scale: Any = None                    # a float for every line prompt, or one float or None per text line; None: 1.0


PAG_ARGUMENTS = ("pag_scale", "pag_applied_layers")


@dataclass
class PerturbedCallExtensions(LineScaleCallExtensions):
    """``LineScaleCallExtensions`` of a call that names a keyword of perturbed-attention guidance (``PAG_ARGUMENTS``).
    ``accepts_call_extensions`` builds it only for such a call."""
    pag_scale: float = 0.0                              # PAG is on iff > 0: v = v_cond + pag_scale · (v_cond − v_perturbed)
    pag_applied_layers: Any = None                      # the blocks whose attention is perturbed, by diffusers module name (``pag_layers``)


def accepts_call_extensions(*names):
    """``__call__`` keeps the reference's parameter list (PIPE:751-781, which ``inspect.signature`` still reports). The fields of
    ``CallExtensions`` in ``names`` are keyword-only extensions of it, taken off here and left on the pipeline, as passed, as
    ``_call_extensions`` for the duration of the call: the only call state that comes from them (what the call derives from them goes to
    ``_denoise`` as an argument). Any other keyword reaches ``__call__`` and its ``TypeError``. Not re-entrant, like the rest of the call state."""
    def decorate(call):
        @functools.wraps(call)
        def wrapper(self, *args, **kwargs):
            taken = {k: kwargs.pop(k) for k in names if k in kwargs}
            record = LineCallExtensions if any(k in LINE_PROMPT_ARGUMENTS for k in taken) else CallExtensions
            if any(k in REGIONAL_IP_ARGUMENTS for k in taken):
                record = RegionalIPCallExtensions
            if any(k in ISOLATION_ARGUMENTS for k in taken):
                record = IsolationCallExtensions
            if any(k in LINE_SCALE_ARGUMENTS for k in taken):
                record = LineScaleCallExtensions
            if any(k in PAG_ARGUMENTS for k in taken):
                record = PerturbedCallExtensions
            self._call_extensions = record(**taken)
            try:
                return call(self, *args, **kwargs)
            finally:
                self._call_extensions = None
        return wrapper
    return decorate


class _StaticFields:          # a ``LoopExtras`` record whose ``STATIC`` names the static inputs of a captured loop that its tensor fields are
    def tensors(self) -> Dict[str, torch.Tensor]:
        return {name: getattr(self, field) for name, field in self.STATIC.items()}

    def rebound(self, static: Dict[str, torch.Tensor]):
        return replace(self, **{field: static[name] for name, field in self.STATIC.items()})


@dataclass(frozen=True)
class UnionTower(_StaticFields):
    """The base flow's second ControlNet in one call: unmasked, evaluated at ``active_steps`` (``union_active_steps``) only."""
    model: FluxControlNetModel
    hint: torch.Tensor
    scale: float
    active_steps: Tuple[int, ...]
    STATIC = {"union_hint": "hint"}

    def signature(self, sig, ident) -> tuple:
        return ("union", ident(self.model), sig(self.hint), self.scale, self.active_steps)


@dataclass(frozen=True)
class Repaint(_StaticFields):
    """Latent-blend repaint: after every step the state becomes ``src32`` re-noised with ``noise32`` to the next sigma where ``mask`` is
    0 and stays the step's result where it is 1 (``scheduler.step_master_(repaint=)``). fp32; under true CFG at the latents' batch B."""
    src32: torch.Tensor       # [B, N, 64] packed source latents
    noise32: torch.Tensor     # [B, N, 64] the noise the start state was mixed with
    mask: torch.Tensor        # [1 or B, N, 64]; fractional values blend
    STATIC = {"repaint_src": "src32", "repaint_noise": "noise32", "repaint_mask": "mask"}

    def signature(self, sig) -> tuple:
        return (("repaint", sig(self.src32), sig(self.noise32), sig(self.mask)),)


@dataclass(frozen=True)
class StepNoise(_StaticFields):
    """The noise streams of a call under stochastic sampling: ``rng`` int64 [B, 2], (seed, subsequence) per sample of the latents' batch
    (``stochastic_rng``). A static input of a captured loop: another seed replays the same graph, which bakes the step index per node."""
    rng: torch.Tensor
    STATIC = {"step_noise_rng": "rng"}


def stochastic_rng(generator, batch: int) -> torch.Tensor:
    """int64 [batch, 2] on the CPU: (seed, subsequence) of every sample's noise stream (csrc/philox.h). A list of generators, one per
    sample: ``(g_b.initial_seed(), 0)``, so sample b of a batch draws what a call of its own with ``g_b`` draws. One generator:
    ``(initial_seed(), b)``. None: one draw from torch's default CPU generator is the seed, with subsequence b. A generator that is
    given is read, never advanced. Seeds are taken modulo 2^64 into the int64's bits."""
    wrap = lambda seed: ((int(seed) + (1 << 63)) % (1 << 64)) - (1 << 63)
    batch = int(batch)
    if isinstance(generator, (list, tuple)):
        if len(generator) != batch:
            raise ValueError(f"a list of {len(generator)} generators for a batch of {batch}")
        rows = [(wrap(g.initial_seed()), 0) for g in generator]
    else:
        seed = int(torch.randint(0, (1 << 63) - 1, (1,), dtype=torch.int64)) if generator is None else wrap(generator.initial_seed())
        rows = [(seed, b) for b in range(batch)]
    return torch.tensor(rows, dtype=torch.int64).reshape(batch, 2)


@dataclass(frozen=True)
class LinePrompts(_StaticFields):
    """Per-line prompts of a call: the transformer's text stream is ``cat([prompt_embeds, embeds], dim=1)`` and its joint
    attention runs with the key groups ``ends`` and the row table ``row_vis`` (``line_prompt_groups``). The towers see the base prompt."""
    embeds: torch.Tensor      # [Bc, R·L, joint_attention_dim]: the R line prompts' T5 embeddings, one after another
    ends: Tuple[int, ...]     # key-group ends over the T0 + R·L + N joint rows
    row_vis: torch.Tensor     # int32 [Bc, T0 + R·L + N]: bit g set = the row sees group g
    STATIC = {"line_embeds": "embeds", "line_row_vis": "row_vis"}

    def groups(self, rows: Optional[slice] = None) -> "ops.KeyGroups":
        return ops.KeyGroups(self.ends, self.row_vis if rows is None else self.row_vis[rows])

    def signature(self, sig) -> tuple:
        return (("line_prompts", self.ends, sig(self.row_vis), sig(self.embeds)),)


def line_prompt_groups(T0: int, L: int, masks, N: int, has_prompt=None, batch: int = 1, cfg: bool = False):
    """The visibility contract of per-line prompts, from host values alone -> (ends, row_vis int32 [batch · (2 if cfg else 1), S]), or
    None when no line has a prompt. ``masks``: one per text line, the regional mask after the pipeline's ÷16 bilinear resize, as [N],
    [1, N, 1] or [batch, N, 1] values; ``has_prompt``: which lines have a prompt (default: all).
    Groups: 0 = the base prompt's T0 tokens; r = 1..R the L tokens of the r-th line THAT HAS A PROMPT; R + 1 = the N image tokens.
    Base text rows see {0, R+1}; line r's text rows see {r, R+1}; image token n sees {0, R+1} and every r whose line's mask is > 0 at n
    (the rule ``active_row_window`` uses for a non-zero row; overlapping boxes OR their bits). Under true CFG the conditioning batch
    is [negative, positive]: the negative half's image rows see {0, R+1} only."""
    has_prompt = [True] * len(masks) if has_prompt is None else [bool(h) for h in has_prompt]
    if len(has_prompt) != len(masks):
        raise ValueError(f"line prompts: {len(has_prompt)} entries for {len(masks)} regional masks")
    lines = [i for i, h in enumerate(has_prompt) if h]
    R = len(lines)
    if R == 0:
        return None
    if R > MAX_LINE_PROMPTS:
        raise ValueError(f"at most {MAX_LINE_PROMPTS} line prompts are supported, got {R}")
    if T0 < 64 or T0 % 64 or L < 64 or L % 64:
        raise ValueError(f"line prompts: the base prompt's length ({T0}) and control_prompt_max_sequence_length ({L}) must be multiples of 64 "
                         "(a 64-key attention tile lies in one group)")
    T = T0 + R * L
    S = T + N
    ends = (T0,) + tuple(T0 + r * L for r in range(1, R + 1)) + (S,)
    img = 1 << (R + 1)
    vis = np.full((batch * (2 if cfg else 1), S), 1 | img, dtype=np.uint32)
    for r, line in enumerate(lines, start=1):
        vis[:, T0 + (r - 1) * L : T0 + r * L] = (1 << r) | img
        on = torch.as_tensor(masks[line]).detach().to("cpu", torch.float32).reshape(-1, N).numpy() > 0      # [1 or batch, N]
        if on.shape[0] not in (1, batch):
            raise ValueError(f"line prompts: regional mask {line} has {on.shape[0]} entries for a batch of {batch}")
        vis[-batch:, T:] |= np.where(on, np.uint32(1 << r), np.uint32(0))
    return ends, torch.from_numpy(vis.view(np.int32))


@dataclass(frozen=True)
class IsolatedLinePrompts(LinePrompts):
    """``LinePrompts`` of a call with ``control_prompt_isolation=True``: the joint attention runs per key (``ops.KeyClasses``) under the
    tables of ``line_prompt_classes``; ``row_vis`` is that rule's. ``ends`` stays what ``line_prompt_groups`` gives (the text layout)."""
    key_class: torch.Tensor             # uint8 [Bc, T0 + R·L + N]: the class of every key
    STATIC = dict(LinePrompts.STATIC, line_key_class="key_class")

    def groups(self, rows: Optional[slice] = None) -> "ops.KeyClasses":
        return ops.KeyClasses(self.row_vis, self.key_class) if rows is None else ops.KeyClasses(self.row_vis[rows], self.key_class[rows])

    def signature(self, sig) -> tuple:
        return LinePrompts.signature(self, sig) + (("line_isolation", sig(self.key_class)),)


def line_prompt_classes(T0: int, L: int, masks, N: int, has_prompt=None, batch: int = 1, cfg: bool = False):
    """The visibility contract of per-line prompts with region isolation, from host values alone -> (row_vis int32 [Bc, S], key_class
    uint8 [Bc, S]), Bc = batch · (2 if cfg else 1), or None when no line has a prompt. Arguments as ``line_prompt_groups``; membership
    of an image token in line r's box is its rule (the resized mask is > 0).
    Key classes: 0 = the base prompt's T0 tokens; r = 1..R the L tokens of the r-th line that has a prompt; then one class per distinct
    MEMBERSHIP SET of the image tokens: R + 1 = in no box (the background; it exists whether or not a token is in it), then the sets
    that occur anywhere in the batch, ascending by their bit mask (bit r - 1 = in box r) — "in box r only", and one class per overlap
    that occurs. More than 32 classes in all raise ``ValueError``.
    Rows: base text rows see 0 and every image class; line r's text rows see r and the image classes whose set contains r (the line's own
    box); an image row in no box sees 0 and every image class; an image row inside boxes M sees 0, every r in M, the background and every
    image class whose set intersects M — not the image keys that lie only in other lines' boxes. Under true CFG the conditioning batch
    is [negative, positive] and the key classes of the negative half are the positive half's; its image rows see 0 and every image class.
    Every row sees at least one key (asserted)."""
    has_prompt = [True] * len(masks) if has_prompt is None else [bool(h) for h in has_prompt]
    if len(has_prompt) != len(masks):
        raise ValueError(f"line prompts: {len(has_prompt)} entries for {len(masks)} regional masks")
    lines = [i for i, h in enumerate(has_prompt) if h]
    R = len(lines)
    if R == 0:
        return None
    if R + 2 > MAX_KEY_CLASSES:
        raise ValueError(f"line prompt isolation: {R} line prompts need more than {MAX_KEY_CLASSES} key classes")
    if T0 < 1 or L < 1 or N < 1:
        raise ValueError(f"line prompts: need at least one base, line and image token, got {T0}, {L}, {N}")
    T = T0 + R * L
    S = T + N
    member = np.zeros((batch, N), dtype=np.int64)                    # bit r - 1: the token lies in box r
    for r, line in enumerate(lines, start=1):
        on = torch.as_tensor(masks[line]).detach().to("cpu", torch.float32).reshape(-1, N).numpy() > 0      # [1 or batch, N]
        if on.shape[0] not in (1, batch):
            raise ValueError(f"line prompts: regional mask {line} has {on.shape[0]} entries for a batch of {batch}")
        member |= np.where(on, np.int64(1 << (r - 1)), np.int64(0))
    sets = [0] + sorted(int(m) for m in np.unique(member) if m != 0)
    if 1 + R + len(sets) > MAX_KEY_CLASSES:
        raise ValueError(f"line prompt isolation: the base prompt, {R} line prompts and {len(sets)} kinds of image token (the background, the "
                         f"boxes and their overlaps) need {1 + R + len(sets)} key classes, at most {MAX_KEY_CLASSES} are supported")
    cls_of = {m: R + 1 + i for i, m in enumerate(sets)}
    img_all = sum(1 << c for c in cls_of.values())
    key_class = np.zeros((batch, S), dtype=np.uint8)
    row_vis = np.full((batch * (2 if cfg else 1), S), 1 | img_all, dtype=np.uint32)
    for r in range(1, R + 1):
        key_class[:, T0 + (r - 1) * L : T0 + r * L] = r
        row_vis[:, T0 + (r - 1) * L : T0 + r * L] = (1 << r) | sum(1 << c for m, c in cls_of.items() if (m >> (r - 1)) & 1)
    word_of = {m: (1 | img_all) if m == 0 else (1 | (m << 1) | (1 << cls_of[0]) | sum(1 << c for m2, c in cls_of.items() if m2 & m)) for m in sets}
    key_class[:, T:] = np.vectorize(cls_of.get, otypes=[np.uint8])(member)
    row_vis[-batch:, T:] = np.vectorize(word_of.get, otypes=[np.uint32])(member)
    if cfg:
        key_class = np.concatenate([key_class, key_class])
    present = np.zeros(key_class.shape[0], dtype=np.uint32)
    for c in range(MAX_KEY_CLASSES):
        present |= np.where((key_class == c).any(axis=1), np.uint32(1 << c), np.uint32(0))
    assert ((row_vis & present[:, None]) != 0).all(), "line_prompt_classes: a row sees no key"
    return torch.from_numpy(row_vis.view(np.int32)), torch.from_numpy(key_class)


@dataclass(frozen=True)
class LineScale(_StaticFields):
    """The strengths of a call's per-line prompts (``control_prompt_scale``) as the joint attention takes them: ``key_bias``
    = ``line_prompt_bias``'s table, ln w_r on key class r. With it the transformer's joint attention runs the biased launch of its rule
    (grouped or keyed). A static input of a captured loop: other values replay the same graph."""
    key_bias: torch.Tensor              # fp32 [1, 32]
    STATIC = {"line_key_bias": "key_bias"}

    def signature(self, sig) -> tuple:
        return (("line_scale", sig(self.key_bias)),)


def line_prompt_bias(scales, has_prompt) -> torch.Tensor:
    """The rule of ``control_prompt_scale``, from host values alone -> fp32 [1, 32]: entry r = ln w_r for the r-th line THAT HAS A PROMPT
    (r = 1..R, numbered as ``line_prompt_groups`` and ``line_prompt_classes`` both number them: classes 1..R are the line tokens under
    either rule, so one table serves both), every other entry 0. ``scales``: one per text line, a float or None (= 1.0); ``has_prompt``:
    which lines have a prompt. The softmax weight of line r's tokens is multiplied by w_r wherever they are visible; who sees them is the
    row tables' matter alone. Under true CFG nothing more is needed: the negative half's image rows do not see the line classes."""
    scales, has_prompt = list(scales), [bool(h) for h in has_prompt]
    if len(scales) != len(has_prompt):
        raise ValueError(f"line prompt scales: {len(scales)} entries for {len(has_prompt)} text lines")
    lines = [i for i, h in enumerate(has_prompt) if h]
    if len(lines) > MAX_LINE_PROMPTS:
        raise ValueError(f"at most {MAX_LINE_PROMPTS} line prompts are supported, got {len(lines)}")
    table = np.zeros((1, MAX_KEY_CLASSES), dtype=np.float32)
    for r, line in enumerate(lines, start=1):
        w = 1.0 if scales[line] is None else float(scales[line])
        if not (math.isfinite(w) and LINE_SCALE_RANGE[0] <= w <= LINE_SCALE_RANGE[1]):
            raise ValueError(f"line prompt scales: a scale lies in [1/64, 64], got {w}")
        table[0, r] = np.float32(math.log(w))
    return torch.from_numpy(table)


def line_scale_argument(ext, line_entries, n_lines: int) -> Optional[list]:
    """Check ``control_prompt_scale`` of a call (``LINE_SCALE_ARGUMENTS``) -> one float per text line, or None when the call does not name
    it (``None`` names nothing). ``line_entries``: what ``line_prompt_arguments`` returned, whose refusals come first."""
    scale = getattr(ext, "control_prompt_scale", None)
    if scale is None:
        return None
    if line_entries is None:
        raise ValueError("control_prompt_scale needs a per-line prompt (control_prompt / control_prompt_embeds): without one there is "
                         "nothing to weigh")
    number = lambda x: isinstance(x, (int, float)) and not isinstance(x, bool)
    if number(scale):
        scales = [float(scale) if e is not None else 1.0 for e in line_entries]
    elif isinstance(scale, (list, tuple)) and len(scale) == n_lines and all(x is None or number(x) for x in scale):
        scales = [1.0 if x is None else float(x) for x in scale]
    else:
        raise ValueError(f"control_prompt_scale must be a float or a list with a float or None per text line (control_image has {n_lines})")
    for w, e in zip(scales, line_entries):
        if not (math.isfinite(w) and LINE_SCALE_RANGE[0] <= w <= LINE_SCALE_RANGE[1]):
            raise ValueError(f"control_prompt_scale: a scale is finite and lies in [1/64, 64] (below it the line prompt is as good as "
                             f"hidden, above it the only text its box sees), got {w}")
        if e is None and w != 1.0:
            raise ValueError(f"control_prompt_scale: a text line without a prompt cannot have a scale ({w}); pass None or 1.0 for it")
    return scales


@dataclass(frozen=True)
class Perturbed(_StaticFields):
    """Perturbed-attention guidance of a call (``pag_scale``): at a guided step the conditioning batch is [perturbed,
    positive], and the joint attention of the double blocks ``double_ids`` and the single blocks ``single_ids`` of the transformer runs
    per key under the tables of ``perturbed_attention_tables`` with the self rule (``ops.attention(self_key=True)``). Every other block,
    the towers, and a guider's unguided steps (the positive half alone, at batch B) run without tables. Two static inputs of a captured loop."""
    row_vis: torch.Tensor               # int32 [2B, T + N]
    key_class: torch.Tensor             # uint8 [1, T + N]
    double_ids: frozenset
    single_ids: frozenset
    STATIC = {"pag_row_vis": "row_vis", "pag_key_class": "key_class"}

    def groups(self) -> "ops.KeyClasses":
        return ops.KeyClasses(self.row_vis, self.key_class)

    def signature(self, sig) -> tuple:
        layers = tuple([f"transformer_blocks.{i}" for i in sorted(self.double_ids)]
                       + [f"single_transformer_blocks.{i}" for i in sorted(self.single_ids)])
        return (("pag", layers, sig(self.row_vis), sig(self.key_class)),)


def pag_layers(names, n_double: int, n_single: int) -> Tuple[frozenset, frozenset]:
    """``pag_applied_layers`` -> (indices of the double blocks, indices of the single blocks). ``names``: a list of the models' diffusers
    module names, ``"transformer_blocks.<i>"`` with i < ``n_double`` and ``"single_transformer_blocks.<i>"`` with i < ``n_single``.
    Anything else, an index out of range, a duplicate and an empty list raise ``ValueError``. There is no default set: which blocks
    are good ones can only be measured with a real checkpoint."""
    if isinstance(names, str) or not isinstance(names, (list, tuple)):
        raise ValueError("pag_applied_layers must be a list of block names such as 'transformer_blocks.8'")
    if len(names) == 0:
        raise ValueError("pag_applied_layers is empty: name at least one block (there is no default set)")
    found = {"transformer_blocks": set(), "single_transformer_blocks": set()}
    limit = {"transformer_blocks": int(n_double), "single_transformer_blocks": int(n_single)}
    for name in names:
        kind, dot, index = name.rpartition(".") if isinstance(name, str) else ("", "", "")
        if kind not in found or not dot or not (index.isascii() and index.isdigit()) or str(int(index)) != index:
            raise ValueError(f"pag_applied_layers: {name!r} is neither 'transformer_blocks.<i>' nor 'single_transformer_blocks.<i>'")
        i = int(index)
        if i >= limit[kind]:
            raise ValueError(f"pag_applied_layers: {name!r} is out of range, the model has {limit[kind]} {kind}")
        if i in found[kind]:
            raise ValueError(f"pag_applied_layers: {name!r} is named twice")
        found[kind].add(i)
    return frozenset(found["transformer_blocks"]), frozenset(found["single_transformer_blocks"])


def perturbed_attention_tables(T: int, N: int, batch: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """The visibility contract of perturbed-attention guidance, from host values alone -> (row_vis int32 [2·batch, T + N], key_class uint8
    [1, T + N]) for the launch with the self rule (``ops.attention(self_key=True)``). Key classes: 0 = the T text keys, 1 = the N image
    keys. Entries [0, batch) are the perturbed half: a text row sees both classes (0b11), an image row class 0 alone (0b01) — the text
    keys, and its own key through the self rule. Entries [batch, 2·batch) are the positive half: every row 0b11. This is diffusers'
    ``PAGJointAttnProcessor2_0`` (recalled) restated for text rows first."""
    T, N, batch = int(T), int(N), int(batch)
    if T < 0 or N < 0 or T + N < 1 or batch < 1:
        raise ValueError(f"perturbed attention tables: need token counts >= 0 with a row in all and a batch >= 1, got T={T}, N={N}, batch={batch}")
    key_class = np.zeros((1, T + N), dtype=np.uint8)
    key_class[0, T:] = 1
    row_vis = np.full((2 * batch, T + N), 0b11, dtype=np.uint32)
    row_vis[:batch, T:] = 0b01
    return torch.from_numpy(row_vis.view(np.int32)), torch.from_numpy(key_class)


def pag_arguments(ext, transformer, cfg: bool) -> Optional[tuple]:
    """Check ``pag_scale`` / ``pag_applied_layers`` of a call (``PAG_ARGUMENTS``), host values only -> (1 + pag_scale formed in double,
    double block indices, single block indices), or None when PAG is off (``pag_scale`` 0: layers that are named are still checked).
    ``cfg``: the call runs true CFG."""
    scale, layers = getattr(ext, "pag_scale", 0.0), getattr(ext, "pag_applied_layers", None)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or scale < 0:
        raise ValueError(f"pag_scale must be a finite number >= 0, got {scale!r}")
    ids = None if layers is None else pag_layers(layers, len(transformer.transformer_blocks), len(transformer.single_transformer_blocks))
    if not scale > 0:
        return None
    if ids is None:
        raise ValueError("pag_scale > 0 needs pag_applied_layers: name the blocks whose attention is perturbed (there is no default set)")
    if cfg:
        raise ValueError("pag_scale cannot be combined with a negative prompt (true CFG): the three-way batch is not supported")
    named = [k for k in LINE_PROMPT_ARGUMENTS[:2] + ("control_prompt_scale", "control_ip_adapter_image", "control_ip_adapter_image_embeds")
             if getattr(ext, k, None) is not None] + (["control_prompt_isolation"] if getattr(ext, "control_prompt_isolation", False) else [])
    if named:
        raise ValueError(f"pag_scale cannot be combined with per-line prompts ({', '.join(named)}): one set of tables per attention launch")
    if getattr(transformer, "_fp8_attention", False):
        raise ValueError("pag_scale needs the bf16 attention kernel: the e4m3 attention (enable_fp8_attention) has no mask")
    return 1.0 + float(scale), ids[0], ids[1]


def line_isolation_argument(ext, line_entries) -> bool:
    """Check ``control_prompt_isolation`` of a call (``ISOLATION_ARGUMENTS``) -> whether its line prompts run under ``line_prompt_classes``."""
    on = getattr(ext, "control_prompt_isolation", False)
    if not isinstance(on, bool):
        raise ValueError(f"control_prompt_isolation must be a bool, got {type(on).__name__}")
    if on and line_entries is None:
        raise ValueError("control_prompt_isolation=True needs a per-line prompt (control_prompt / control_prompt_embeds): without one there "
                         "is nothing to isolate")
    return on


def line_prompt_arguments(ext, n_lines: int, control_mask, fp8_attention: bool = False) -> Optional[list]:
    """Check the per-line prompt keywords of a call -> one entry per text line (a string, a [B, L, D] tensor or None), or None when
    the call names none."""
    prompts, embeds = getattr(ext, "control_prompt", None), getattr(ext, "control_prompt_embeds", None)
    if prompts is None and embeds is None:
        return None
    if prompts is not None and embeds is not None:
        raise ValueError("pass control_prompt or control_prompt_embeds, not both")
    entries = prompts if prompts is not None else embeds
    name = "control_prompt" if prompts is not None else "control_prompt_embeds"
    if not isinstance(entries, (list, tuple)) or len(entries) != n_lines:
        raise ValueError(f"{name} must be a list with one entry per text line (control_image has {n_lines}), a {'string' if prompts is not None else 'tensor'} or None each")
    L = ext.control_prompt_max_sequence_length
    if not isinstance(L, int) or L < 64 or L % 64 or L > 512:
        raise ValueError(f"control_prompt_max_sequence_length must be a multiple of 64 and at most 512, got {L}")
    for e in entries:
        if e is not None and not isinstance(e, str if prompts is not None else torch.Tensor):
            raise ValueError(f"{name}: an entry is a {'string' if prompts is not None else 'tensor'} or None, got {type(e).__name__}")
        if isinstance(e, torch.Tensor) and (e.dim() != 3 or e.shape[1] != L):
            raise ValueError(f"control_prompt_embeds: an entry is [B, {L}, joint_attention_dim] (control_prompt_max_sequence_length rows), got {tuple(e.shape)}")
    if sum(e is not None for e in entries) > MAX_LINE_PROMPTS:
        raise ValueError(f"at most {MAX_LINE_PROMPTS} line prompts are supported, got {sum(e is not None for e in entries)}")
    if all(e is None for e in entries):
        return None
    if control_mask is None or len(control_mask) != n_lines:
        raise ValueError(f"{name} needs control_mask: a line's prompt is visible to the image tokens inside that line's regional mask")
    if fp8_attention:
        raise ValueError(f"{name} cannot be combined with enable_fp8_attention: the e4m3 attention kernel takes no mask "
                         "(the e4m3 linear levels with bf16 attention are fine)")
    return list(entries)


@dataclass(frozen=True)
class RegionalIP:
    """The image prompts of a call that has a regional one, as ordered terms through the one loaded adapter: the call's
    own prompt first, if given, then the text lines' in order. Each later term adds with one more rounding: the order is the contract of
    the bits. Weights as ``ip_adapter.regional_ip_weights`` makes them; (None, None) = the call's own prompt without a mask."""
    embeds: Tuple[torch.Tensor, ...]                    # per term [Bc or 1, E] bf16
    img_w: Tuple[Optional[torch.Tensor], ...]           # per term fp32 [Bc or 1, N], or None
    txt_w: Tuple[Optional[torch.Tensor], ...]           # per term fp32 [Bc or 1] (the text rows of an InstantX single block), or None

    def signature(self, sig) -> tuple:
        return ("regional_ip", len(self.embeds), tuple(w is not None for w in self.img_w), tuple(sig(e) for e in self.embeds),
                tuple(None if w is None else sig(w) for w in self.img_w))

    def tensors(self) -> Dict[str, torch.Tensor]:
        """The static inputs of a captured loop, by name."""
        out = {f"rip_embeds{i}": e for i, e in enumerate(self.embeds)}
        out.update({f"rip_img_w{i}": w for i, w in enumerate(self.img_w) if w is not None})
        out.update({f"rip_txt_w{i}": w for i, w in enumerate(self.txt_w) if w is not None})
        return out

    def rebound(self, static: Dict[str, torch.Tensor]) -> "RegionalIP":
        n = range(len(self.embeds))
        return RegionalIP(tuple(static[f"rip_embeds{i}"] for i in n), tuple(static.get(f"rip_img_w{i}") for i in n),
                          tuple(static.get(f"rip_txt_w{i}") for i in n))


def regional_ip_arguments(ext, n_lines: int, control_mask, adapter, positive_ip: bool, has_encoder: bool):
    """Check the regional image prompt keywords of a call (``REGIONAL_IP_ARGUMENTS``) -> None when the call names none, else
    (one entry per text line: an image, an embedding [B or 1, E] or None; one scale per line; the call's ``ip_adapter_mask`` or None)."""
    mask = getattr(ext, "ip_adapter_mask", None)
    images, embeds = getattr(ext, "control_ip_adapter_image", None), getattr(ext, "control_ip_adapter_image_embeds", None)
    if mask is None and images is None and embeds is None:
        return None
    if images is not None and embeds is not None:
        raise ValueError("pass control_ip_adapter_image or control_ip_adapter_image_embeds, not both")
    if adapter is None:
        raise ValueError("ip_adapter_mask / control_ip_adapter_image / control_ip_adapter_image_embeds were passed but no IP-Adapter is "
                         "loaded (load_ip_adapter)")
    if mask is not None and not positive_ip:
        raise ValueError("`ip_adapter_mask` was passed without an image prompt (ip_adapter_image / ip_adapter_image_embeds)")
    entries = images if images is not None else embeds
    name = "control_ip_adapter_image" if images is not None else "control_ip_adapter_image_embeds"
    if entries is None:
        return [None] * n_lines, [1.0] * n_lines, mask
    if not isinstance(entries, (list, tuple)) or len(entries) != n_lines:
        raise ValueError(f"{name} must be a list with one entry per text line (control_image has {n_lines}), "
                         f"{'an image' if images is not None else 'a tensor'} or None each")
    out = []
    for e in entries:
        if e is None:
            out.append(None)
        elif images is not None:
            import PIL.Image

            if not isinstance(e, (PIL.Image.Image, np.ndarray, torch.Tensor)):
                raise ValueError(f"{name}: an entry is an image (PIL, array or pixel tensor) or None, got {type(e).__name__}")
            out.append(e)
        else:
            if not isinstance(e, torch.Tensor) or e.dim() not in (2, 3) or (e.dim() == 3 and e.shape[1] != 1):
                raise ValueError(f"{name}: an entry is a [B,1,E], [B,E] or [1,E] tensor or None, got "
                                 f"{tuple(e.shape) if isinstance(e, torch.Tensor) else type(e).__name__}")
            e = e[:, 0] if e.dim() == 3 else e
            if e.shape[1] != adapter.E:
                raise ValueError(f"{name}: width {e.shape[1]} != the adapter's image embedding width {adapter.E}")
            out.append(e)
    scale = getattr(ext, "control_ip_adapter_scale", 1.0)
    if isinstance(scale, (int, float)):
        scales = [float(scale)] * n_lines
    elif isinstance(scale, (list, tuple)) and len(scale) == n_lines and all(isinstance(x, (int, float)) for x in scale):
        scales = [float(x) for x in scale]
    else:
        raise ValueError(f"control_ip_adapter_scale must be a float or one float per text line ({n_lines})")
    if any(e is not None for e in out):
        if control_mask is None or len(control_mask) != n_lines:
            raise ValueError(f"{name} needs control_mask: a line's image prompt is confined to that line's regional mask")
        if images is not None and not has_encoder:
            raise NotImplementedError(f"{name} needs an image encoder, which this pipeline does not have: encode the image yourself and "
                                      "pass control_ip_adapter_image_embeds")
    return out, scales, mask


@dataclass(frozen=True)
class LoopExtras:
    """What a call adds to the plain loop of ``_denoise_eager``. ``_denoise`` sets ``tower_window`` itself; what the fields add to a captured
    graph (key, static inputs, the capture's own extras) their records say: ``signature``, ``tensors()``, ``rebound(static)``, walked below."""
    ip_embeds: Optional[torch.Tensor] = None     # the image prompt, [total or 1, E] ([2·total, E] under true CFG); None: nothing to add
    union: Optional[UnionTower] = None           # it keeps the side stream and the text towers' row window
    # true CFG of the base flow: the conditioning batch is [negative, positive] (2B against the latents' B) and the step mixes its halves in
    # fp32 (``scheduler.step_master_(v_text=, s=)``); all else sees Bc = 2B
    cfg_scale: Optional[float] = None
    tower_window: Any = None                     # ``active_row_window`` of the masks from the call prologue (None: every row)
    # (FluxControlNetModel, hint, conditioning scale) of unmasked towers after the text lines (the inpaint tower); the loop then stays on one stream
    extra_towers: Tuple = ()
    velocity: Optional[Callable] = None          # (i, noise_pred) -> what the scheduler steps with in its place (the inpaint flow's CFG)
    repaint: Optional[Repaint] = None            # the step also blends the re-noised source back in (pipeline_repaint.py)
    # under true CFG, a guider that changes the call (guidance.Guidance: the guider and the steps it guides): projected guidance at
    # those steps, and the steps outside them run on the positive half alone, at the latents' batch B; None: every step is the CFG step
    guidance: Optional[Guidance] = None
    line_prompts: Optional[LinePrompts] = None   # per-line prompts: a longer text stream and key groups for the transformer alone
    regional_ip: Optional[RegionalIP] = None     # regional image prompts; it then holds the call's own prompt too, and ip_embeds is None
    # pag_scale: cfg_scale is 1 + pag_scale and the first half of the conditioning batch is the positive one under the perturbed tables
    # (never together with line_prompts / line_scale; its key part is the last)
    perturbed: Optional[Perturbed] = None
    # stochastic sampling (the scheduler's switch): the noise streams of the call's samples for ``scheduler.step_master_(stochastic=)``;
    # its key part, ("stochastic", eta), is appended by ``_graph_signature`` after everything else
    step_noise: Optional[StepNoise] = None
    line_scale: Optional[LineScale] = None      # control_prompt_scale: a bias per key class for the joint attention of line_prompts
    quiet: bool = False                          # no progress bar (a capture)

    def signature(self, sig, ident, adapter) -> tuple:
        """The extensions' part of a captured graph's key, one row per field in field order; an absent field adds nothing."""
        ip = adapter is not None and (adapter.version, tuple(adapter.scales))      # of either kind of image prompt: kernel scalars
        return ((() if self.ip_embeds is None else (sig(self.ip_embeds),) + ip)
                + (() if self.union is None else self.union.signature(sig, ident))
                + (() if self.cfg_scale is None else (("cfg", self.cfg_scale),))
                + (() if self.repaint is None else self.repaint.signature(sig))
                + (() if self.guidance is None else self.guidance.signature())
                + (() if self.line_prompts is None else self.line_prompts.signature(sig))
                + (() if self.regional_ip is None else (self.regional_ip.signature(sig),) + ip)
                + (() if self.line_scale is None else self.line_scale.signature(sig))
                + (() if self.perturbed is None else self.perturbed.signature(sig)))

    def tensors(self) -> Dict[str, torch.Tensor]:          # the static inputs the fields add, in the order they are cloned and refreshed
        records = [getattr(self, f.name) for f in fields(self)]      # one with static inputs of its own is known by its ``tensors`` method
        own = {} if self.ip_embeds is None else {"ip_embeds": self.ip_embeds}
        return dict(own, **{name: t for r in records if hasattr(r, "tensors") for name, t in r.tensors().items()})

    def rebound(self, static: Dict[str, torch.Tensor]) -> "LoopExtras":          # what a capture runs with: the graph's own clones, no progress bar
        own = {f.name: getattr(self, f.name).rebound(static) for f in fields(self) if hasattr(getattr(self, f.name), "tensors")}
        return replace(self, quiet=True, ip_embeds=static.get("ip_embeds"), **own)

    def kept(self, transformer) -> list:     # what a captured graph reads besides its static inputs and the pipeline's own models
        union = [] if self.union is None else [self.union.model._ensure_plans(), getattr(self.union.model, "_cx_pad", None)]
        return [getattr(transformer, "_ip_adapter", None) if self.ip_embeds is not None or self.regional_ip is not None else None] + union


def do_true_cfg(true_cfg_scale, negative_prompt=None, negative_prompt_embeds=None, negative_pooled_prompt_embeds=None) -> bool:
    """diffusers' rule (recalled): a scale above 1 AND a negative prompt, as text or as both embeddings."""
    has_negative = negative_prompt is not None or (negative_prompt_embeds is not None and negative_pooled_prompt_embeds is not None)
    return bool(float(true_cfg_scale) > 1 and has_negative)


class FluxControlNetPipeline:
    model_cpu_offload_seq = "text_encoder->text_encoder_2->transformer->vae"
    _optional_components: List[str] = []
    _callback_tensor_inputs = ["latents", "prompt_embeds"]

    def __init__(self, scheduler: FlowMatchEulerDiscreteScheduler, vae: AutoencoderKL, text_encoder, tokenizer, text_encoder_2,
                 tokenizer_2, transformer: FluxTransformer2DModel,
                 controlnet: Union[FluxControlNetModel, List[FluxControlNetModel], Tuple[FluxControlNetModel], FluxMultiControlNetModel]):
        self.vae, self.text_encoder, self.text_encoder_2 = vae, text_encoder, text_encoder_2
        self.tokenizer, self.tokenizer_2 = tokenizer, tokenizer_2
        self.transformer, self.scheduler, self.controlnet = transformer, scheduler, controlnet
        self.vae_scale_factor = 2 ** len(self.vae.config.block_out_channels) if self.vae is not None else 16       # Q9
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor)
        self.tokenizer_max_length = self.tokenizer.model_max_length if self.tokenizer is not None else 77
        self.default_sample_size = 64
        self._guidance_scale, self._joint_attention_kwargs, self._interrupt, self._num_timesteps = 1.0, None, False, 0
        self._progress_disabled = False
        self._call_extensions: Optional[CallExtensions] = None          # set by accepts_call_extensions while a call runs
        # the IP-Adapter's image side (image_encoder.py); set by from_pretrained / load_ip_adapter or assigned, not components
        self.image_encoder, self.feature_extractor = None, None
        # a second, unmasked ControlNet with its own step window beside the text-line tower (Union-Pro-2.0: canny / depth / pose); set
        # by from_pretrained(controlnet_union=) or assigned, fed by __call__(control_image_union=...) — base pipeline only
        self.controlnet_union: Optional[FluxControlNetModel] = None
        # what a true-CFG call adds to the plain mix at every step: a guidance interval and projected guidance (guidance.TrueCFGGuider);
        # assigned, read by a call with a negative prompt — not a component, not saved
        self.guider = None

    # ------------------------------------------------------------------ component plumbing
    @property
    def components(self) -> Dict[str, Any]:
        c = dict(scheduler=self.scheduler, vae=self.vae, text_encoder=self.text_encoder, tokenizer=self.tokenizer,
                 text_encoder_2=self.text_encoder_2, tokenizer_2=self.tokenizer_2, transformer=self.transformer,
                 controlnet=self.controlnet)
        if self.controlnet_union is not None:
            c["controlnet_union"] = self.controlnet_union
        return c

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, controlnet=None, torch_dtype=None, **kwargs):
        """Loader in the diffusers layout (``model_index.json`` + one sub-folder per component), as
        infer.py:31-33 calls it. ``pretrained_model_name_or_path`` is a local directory or a hub id that resolves through the
        LOCAL hub cache (modules.resolve_model_path: ``$HF_HOME/hub/models--ORG--NAME/snapshots/…``; nothing is downloaded).
        ``model_index.json`` decides which components exist: the text encoders load into reptext_amd.text_encoders (HIP
        kernels) and the tokenizers through `transformers` when listed and present; else they stay None and the caller
        passes ``prompt_embeds``/``pooled_prompt_embeds``. Components passed as keyword arguments are taken as they are."""
        from .modules import resolve_model_path

        root = resolve_model_path(pretrained_model_name_or_path, kwargs.pop("revision", None))
        dt = torch_dtype or torch.bfloat16
        index = {}
        ip = os.path.join(root, "model_index.json")
        if os.path.isfile(ip):
            with open(ip) as f:
                index = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
        listed = lambda name: (not index) or (index.get(name) not in (None, [None, None]))
        for required in ("transformer", "vae"):
            if required not in kwargs and not (listed(required) and os.path.isdir(os.path.join(root, required))):
                raise OSError(f"{cls.__name__}.from_pretrained: component '{required}' is neither passed nor present under {root}")
        sched_cfg, sched_name = {}, None
        sp = os.path.join(root, "scheduler", "scheduler_config.json")
        if os.path.isfile(sp):
            with open(sp) as f:
                saved = json.load(f)
            sched_cfg, sched_name = {k: v for k, v in saved.items() if not k.startswith("_")}, saved.get("_class_name")
        # the file's _class_name picks one of the two schedulers; any other name (a diffusers scheduler this package does not have)
        # keeps the Euler class with the keys it knows
        sched_cls = {c.__name__: c for c in (FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler)}.get(sched_name)
        if sched_cls is None:
            if sched_name is not None and "scheduler" not in kwargs:
                import sys
                print(f"[reptext_amd] scheduler class {sched_name!r} is not available; using FlowMatchEulerDiscreteScheduler", file=sys.stderr, flush=True)
            sched_cls = FlowMatchEulerDiscreteScheduler
        known = set(sched_cls().config.keys()) | set(STOCHASTIC_DEFAULTS)
        scheduler = kwargs.pop("scheduler", None) or sched_cls(**{k: v for k, v in sched_cfg.items() if k in known})
        transformer = kwargs.pop("transformer", None) or FluxTransformer2DModel.from_pretrained(root, torch_dtype=dt, subfolder="transformer")
        vae = kwargs.pop("vae", None) or AutoencoderKL.from_pretrained(root, torch_dtype=dt, subfolder="vae")
        te, te2 = kwargs.pop("text_encoder", None), kwargs.pop("text_encoder_2", None)
        tok, tok2 = kwargs.pop("tokenizer", None), kwargs.pop("tokenizer_2", None)
        image_encoder, feature_extractor = kwargs.pop("image_encoder", None), kwargs.pop("feature_extractor", None)
        if image_encoder is None and index.get("image_encoder") not in (None, [None, None]) and os.path.isdir(os.path.join(root, "image_encoder")):
            from .image_encoder import image_encoder_class

            image_encoder = image_encoder_class(os.path.join(root, "image_encoder")).from_pretrained(root, subfolder="image_encoder", torch_dtype=dt)
        try:
            if te is None and listed("text_encoder") and os.path.isdir(os.path.join(root, "text_encoder")):
                from .text_encoders import CLIPTextModel                 # the encoders themselves run on the HIP kernels

                te = CLIPTextModel.from_pretrained(root, subfolder="text_encoder", torch_dtype=dt)
            if te2 is None and listed("text_encoder_2") and os.path.isdir(os.path.join(root, "text_encoder_2")):
                from .text_encoders import T5EncoderModel

                te2 = T5EncoderModel.from_pretrained(root, subfolder="text_encoder_2", torch_dtype=dt)
            if tok is None and listed("tokenizer") and os.path.isdir(os.path.join(root, "tokenizer")):
                from transformers import CLIPTokenizer                   # tokenisation is host-side string work

                tok = CLIPTokenizer.from_pretrained(os.path.join(root, "tokenizer"))
            if tok2 is None and listed("tokenizer_2") and os.path.isdir(os.path.join(root, "tokenizer_2")):
                from transformers import T5TokenizerFast

                tok2 = T5TokenizerFast.from_pretrained(os.path.join(root, "tokenizer_2"))
        except Exception as e:  # pragma: no cover - depends on local files
            raise OSError(f"could not load text encoders from {root}: {e}") from e
        if isinstance(controlnet, str):
            controlnet = FluxControlNetModel.from_pretrained(controlnet, torch_dtype=dt)
        controlnet_union = kwargs.pop("controlnet_union", None)          # a model, a local directory or a cached hub id, like controlnet=
        if isinstance(controlnet_union, str):
            controlnet_union = FluxControlNetModel.from_pretrained(controlnet_union, torch_dtype=dt)
        extra = {k: kwargs[k] for k in ("controlnet_inpaint",) if k in kwargs}
        pipe = cls(scheduler=scheduler, vae=vae, text_encoder=te, tokenizer=tok, text_encoder_2=te2, tokenizer_2=tok2,
                   transformer=transformer, controlnet=controlnet, **extra)
        pipe.image_encoder, pipe.feature_extractor = image_encoder, feature_extractor
        pipe.controlnet_union = controlnet_union
        return pipe

    def save_pretrained(self, root: str, max_shard_bytes: int = 10 << 30) -> None:
        """Write the diffusers layout this class loads: model_index.json, scheduler/scheduler_config.json and one folder per
        model component that has weights here (the ControlNet is a separate repository in the reference and is not part of it)."""
        os.makedirs(root, exist_ok=True)
        index = {"_class_name": type(self).__name__, "_diffusers_version": "0.36.0"}
        for name in ("transformer", "vae", "text_encoder", "text_encoder_2"):
            m = getattr(self, name, None)
            if m is not None and hasattr(m, "save_pretrained"):
                m.save_pretrained(os.path.join(root, name), max_shard_bytes=max_shard_bytes) if name in ("transformer", "vae") else m.save_pretrained(os.path.join(root, name))
                index[name] = ["reptext_amd", type(m).__name__]
            else:
                index[name] = [None, None]
        for name in ("tokenizer", "tokenizer_2"):
            t = getattr(self, name, None)
            if t is not None and hasattr(t, "save_pretrained"):
                t.save_pretrained(os.path.join(root, name))
                index[name] = ["transformers", type(t).__name__]
            else:
                index[name] = [None, None]
        os.makedirs(os.path.join(root, "scheduler"), exist_ok=True)
        with open(os.path.join(root, "scheduler", "scheduler_config.json"), "w") as f:
            json.dump(dict(_class_name=type(self.scheduler).__name__, **dict(self.scheduler.config)), f, indent=2)
        index["scheduler"] = ["reptext_amd", type(self.scheduler).__name__]
        with open(os.path.join(root, "model_index.json"), "w") as f:
            json.dump(index, f, indent=2)

    def to(self, device=None, dtype=None):
        for m in list(self.components.values()) + [self.image_encoder]:
            if isinstance(m, torch.nn.Module):
                m.to(device=device, dtype=dtype) if dtype is not None else m.to(device)
        return self

    @property
    def _execution_device(self):
        return self.transformer.device

    @property
    def device(self):
        return self.transformer.device

    def maybe_free_model_hooks(self):
        """Offload hooks belong to accelerate-based CPU offload, which this single-device path does not use (no-op)."""

    def set_progress_bar_config(self, disable: bool = False, **kw):
        self._progress_disabled = disable

    def progress_bar(self, total=None):
        return _Progress(total, disable=self._progress_disabled)

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def joint_attention_kwargs(self):
        return self._joint_attention_kwargs

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def interrupt(self):
        return self._interrupt

    # ------------------------------------------------------------------ prompt encoding (PIPE:232-456)
    def _require_text_stack(self):
        if self.text_encoder is None or self.text_encoder_2 is None or self.tokenizer is None or self.tokenizer_2 is None:
            raise ValueError("this pipeline was built without text encoders/tokenizers: pass `prompt_embeds` and "
                             "`pooled_prompt_embeds` instead of `prompt`")

    def _get_t5_prompt_embeds(self, prompt, num_images_per_prompt=1, max_sequence_length=512, device=None, dtype=None):
        self._require_text_stack()
        device = device or self._execution_device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        tok = self.tokenizer_2(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                               return_length=False, return_overflowing_tokens=False, return_tensors="pt")
        emb = self.text_encoder_2(tok.input_ids.to(device), output_hidden_states=False)[0]
        emb = emb.to(dtype=self.text_encoder_2.dtype, device=device)
        b, seq, _ = emb.shape
        return emb.repeat(1, num_images_per_prompt, 1).view(b * num_images_per_prompt, seq, -1)

    def _get_clip_prompt_embeds(self, prompt, num_images_per_prompt=1, device=None):
        self._require_text_stack()
        device = device or self._execution_device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        tok = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer_max_length, truncation=True,
                             return_overflowing_tokens=False, return_length=False, return_tensors="pt")
        pooled = self.text_encoder(tok.input_ids.to(device), output_hidden_states=False).pooler_output
        pooled = pooled.to(dtype=self.text_encoder.dtype, device=device)
        return pooled.repeat(1, num_images_per_prompt).view(len(prompt) * num_images_per_prompt, -1)

    def encode_prompt(self, prompt, prompt_2, device=None, num_images_per_prompt: int = 1, prompt_embeds=None,
                      pooled_prompt_embeds=None, max_sequence_length: int = 512, lora_scale=None):
        """Returns (prompt_embeds [B,L,4096], pooled [B,768], text_ids zeros[L,3]) — PIPE:349-456 (LoRA scaling is inert:
        no PEFT on this path)."""
        device = device or self._execution_device
        if prompt_embeds is None:
            prompt = [prompt] if isinstance(prompt, str) else prompt
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            pooled_prompt_embeds = self._get_clip_prompt_embeds(prompt, num_images_per_prompt, device)
            prompt_embeds = self._get_t5_prompt_embeds(prompt_2, num_images_per_prompt, max_sequence_length, device)
        ids_dtype = self.text_encoder.dtype if self.text_encoder is not None else prompt_embeds.dtype
        text_ids = torch.zeros(prompt_embeds.shape[1], 3, device=device, dtype=ids_dtype)
        return prompt_embeds, pooled_prompt_embeds, text_ids

    def _encode_vae_image(self, image: torch.Tensor, generator):
        """PIPE:459-471: sample the posterior (per-sample generators allowed) and apply (z - shift) * scaling."""
        if isinstance(generator, list):
            lat = torch.cat([retrieve_latents(self.vae.encode(image[i : i + 1]), generator=generator[i]) for i in range(image.shape[0])], dim=0)
        else:
            lat = retrieve_latents(self.vae.encode(image), generator=generator)
        return (lat - self.vae.config.shift_factor) * self.vae.config.scaling_factor

    # ------------------------------------------------------------------ validation (PIPE:485-531)
    def check_inputs(self, prompt, prompt_2, height, width, prompt_embeds=None, pooled_prompt_embeds=None,
                     callback_on_step_end_tensor_inputs=None, max_sequence_length=None):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_on_step_end_tensor_inputs is not None:
            bad = [k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]
            if bad:
                raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found {bad}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        if prompt_2 is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt_2`: {prompt_2} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if prompt_2 is not None and not isinstance(prompt_2, (str, list)):
            raise ValueError(f"`prompt_2` has to be of type `str` or `list` but is {type(prompt_2)}")
        if prompt_embeds is not None and pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed. Make sure to generate "
                             "`pooled_prompt_embeds` from the same text encoder that was used to generate `prompt_embeds`.")
        if max_sequence_length is not None and max_sequence_length > 512:
            raise ValueError(f"`max_sequence_length` cannot be greater than 512 but is {max_sequence_length}")

    # ------------------------------------------------------------------ latent helpers (PIPE:533-570)
    @staticmethod
    def _prepare_latent_image_ids(batch_size, height, width, device, dtype):
        """(0,row,col) per token of the (height/2)x(width/2) grid, row-major (height/width are LATENT sizes)."""
        rows = torch.arange(height // 2, dtype=torch.float32)
        cols = torch.arange(width // 2, dtype=torch.float32)
        ids = torch.stack([torch.zeros(height // 2, width // 2), rows[:, None].expand(-1, width // 2),
                           cols[None, :].expand(height // 2, -1)], dim=-1)
        return ids.reshape(-1, 3).to(device=device, dtype=dtype)

    @staticmethod
    def _pack_latents(latents, batch_size, num_channels_latents, height, width):
        """[B,C,H,W] -> [B,(H/2)(W/2),4C] with channel order (c,dy,dx). GPU bf16 tensors use the HIP kernel."""
        if latents.is_cuda and latents.dtype == torch.bfloat16:
            return ops.pack_latents(latents.reshape(batch_size, num_channels_latents, height, width))
        x = latents.reshape(batch_size, num_channels_latents, height // 2, 2, width // 2, 2)
        return x.permute(0, 2, 4, 1, 3, 5).reshape(batch_size, (height // 2) * (width // 2), num_channels_latents * 4)

    @staticmethod
    def _unpack_latents(latents, height, width, vae_scale_factor):
        b, _, ch = latents.shape
        h, w = height // vae_scale_factor, width // vae_scale_factor
        x = latents.reshape(b, h, w, ch // 4, 2, 2).permute(0, 3, 1, 4, 2, 5)
        return x.reshape(b, ch // 4, h * 2, w * 2)

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        h2 = 2 * (int(height) // self.vae_scale_factor)
        w2 = 2 * (int(width) // self.vae_scale_factor)
        ids = self._prepare_latent_image_ids(batch_size, h2, w2, device, dtype)
        if latents is not None:
            return latents.to(device=device, dtype=dtype), ids
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        noise = randn_tensor((batch_size, num_channels_latents, h2, w2), generator=generator, device=device, dtype=dtype)
        return self._pack_latents(noise, batch_size, num_channels_latents, h2, w2), ids

    def _glyph_blend(self, image, image_latents, noise):
        """0.10·glyph latent + noise where the bilinearly down-sampled glyph mask is > 0 (PIPE:645-654). On the GPU one HIP
        kernel (mask, resize, threshold, blend: ops.glyph_blend, bit-identical resize to F.interpolate); torch ops on the CPU."""
        if image.is_cuda:
            return ops.glyph_blend(image.to(torch.float32), image_latents.to(torch.float32), noise.to(torch.float32)).to(noise.dtype)
        m = (image > 0).any(dim=1, keepdim=True).float()
        m = F.interpolate(m, size=noise.shape[-2:], mode="bilinear", align_corners=False) > 0
        return torch.where(m, 0.10 * image_latents + noise, noise)

    glyph_blend_is_initial_latents = False     # Q1; the inpaint pipeline's reference returns the blend (INP:645-647)

    def prepare_latents_reptext(self, image, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        """PIPE:608-660 / INP:598-653. The glyph image is VAE-encoded with `generator` (advancing its stream by one [B,16,h,w]
        normal draw) before the noise is drawn, and 0.10·glyph latent + noise is computed where the down-sampled glyph mask is
        positive. Quirk Q1: this pipeline's reference then drops that blend and returns the plain noise; under
        `glyph_blend_is_initial_latents` the blend is what is returned."""
        h2 = 2 * (int(height) // self.vae_scale_factor)
        w2 = 2 * (int(width) // self.vae_scale_factor)
        image = image.to(device=device, dtype=dtype)
        image_latents = self._encode_vae_image(image=image, generator=generator)
        n_img = image_latents.shape[0]
        if batch_size > n_img and batch_size % n_img == 0:
            image_latents = torch.cat([image_latents] * (batch_size // n_img), dim=0)
        elif batch_size > n_img:
            raise ValueError(f"Cannot duplicate `image` of batch size {n_img} to {batch_size} text prompts.")
        ids = self._prepare_latent_image_ids(batch_size, h2, w2, device, dtype)
        if latents is not None:
            return latents.to(device=device, dtype=dtype), ids
        noise = randn_tensor((batch_size, num_channels_latents, h2, w2), generator=generator, device=device, dtype=dtype)
        blend = self._glyph_blend(image, image_latents, noise)            # computed even where it is dropped, as in the reference (Q1)
        start = blend.to(dtype) if self.glyph_blend_is_initial_latents else noise
        return self._pack_latents(start, batch_size, num_channels_latents, h2, w2), ids

    def _prep_pixels(self, image, width, height, batch_size, num_images_per_prompt, device, dtype, processor=None):
        if not isinstance(image, torch.Tensor):
            image = (processor or self.image_processor).preprocess(image, height=height, width=width)
        repeat_by = batch_size if image.shape[0] == 1 else num_images_per_prompt
        return image.repeat_interleave(repeat_by, dim=0).to(device=device, dtype=dtype)

    def prepare_image(self, image, width, height, batch_size, num_images_per_prompt, device, dtype, image_position=None,
                      do_classifier_free_guidance=False, guess_mode=False):
        """PIPE:663-731: VAE-encode the canny hint and the (3-channel repeated) position hint, concatenate on channels,
        pack -> [B, N, 128]. Both posteriors are sampled from the GLOBAL torch RNG (no generator; quirk Q2)."""
        image = self._prep_pixels(image, width, height, batch_size, num_images_per_prompt, device, dtype)
        pos = self._prep_pixels(image_position, width, height, batch_size, num_images_per_prompt, device, dtype).repeat(1, 3, 1, 1)
        sf, sc = self.vae.config.shift_factor, self.vae.config.scaling_factor
        lat = ((self.vae.encode(image.to(self.vae.dtype)).latent_dist.sample() - sf) * sc).to(dtype)
        plat = ((self.vae.encode(pos.to(self.vae.dtype)).latent_dist.sample() - sf) * sc).to(dtype)
        both = torch.cat([lat, plat], dim=1)
        packed = self._pack_latents(both, batch_size * num_images_per_prompt, both.shape[1], both.shape[2], both.shape[3])
        if do_classifier_free_guidance:
            packed = torch.cat([packed] * 2)
        return packed, height, width

    def _region_masks(self, control_mask, device, dtype) -> List[torch.Tensor]:
        """PIPE:1007-1013: mask/255 -> bilinear x1/16 -> [1, N, 1]. uint8 masks headed for the GPU are divided and resized
        there (ops.resize2d: same source-index rule and fp32 expression order as F.interpolate, bit-identical)."""
        out = []
        if control_mask is not None:
            for m in control_mask:
                if isinstance(m, torch.Tensor) and m.dim() == 3 and m.shape[-1] == 1:
                    out.append(m.to(device=device, dtype=dtype))      # an extension, like packed hints: token masks, one per image [B,N,1]
                    continue
                arr = np.array(m)
                if torch.device(device).type == "cuda" and arr.dtype == np.uint8 and arr.ndim == 2:
                    t = ops.resize2d(torch.from_numpy(arr).to(device)[None, None], scale_factor=1 / 16, mode="bilinear", u8_scale=255.0)
                    out.append(t.reshape([1, -1, 1]).to(dtype))
                    continue
                rm = torch.from_numpy(arr) / 255.0
                t = F.interpolate(rm[None, None].float(), scale_factor=1 / 16, mode="bilinear").reshape([1, -1, 1])
                out.append(t.to(device=device, dtype=dtype))
        return out

    def _is_packed_hint(self, t, tower=None) -> bool:
        cn = tower if tower is not None else self.controlnet
        return isinstance(t, torch.Tensor) and t.dim() == 3 and isinstance(cn, FluxControlNetModel) and \
            t.shape[-1] == cn.controlnet_x_embedder.weight.shape[1]

    # ------------------------------------------------------------------ LoRA: the FluxLoraLoaderMixin subset (PIPE:15,163), routed to
    # the transformer; adapters are merged into the bf16 weights on the device (lora.py), so the loop and its graph are unchanged
    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, adapter_name: Optional[str] = None, weight_name: Optional[str] = None,
                          **kwargs):
        self.transformer.load_lora_adapter(pretrained_model_name_or_path_or_dict, adapter_name=adapter_name, weight_name=weight_name,
                                           prefix="transformer")

    def set_adapters(self, adapter_names, adapter_weights=None):
        self.transformer.set_adapters(adapter_names, adapter_weights)

    def get_active_adapters(self) -> List[str]:
        return self.transformer.active_adapters()

    def get_list_adapters(self) -> Dict[str, List[str]]:
        m = getattr(self.transformer, "_lora", None)
        return {} if m is None or not m.state.adapters else {"transformer": sorted(m.state.adapters)}

    def fuse_lora(self, lora_scale: float = 1.0, adapter_names=None, **kwargs):
        self.transformer.fuse_lora(lora_scale, adapter_names)

    def unfuse_lora(self, **kwargs):
        self.transformer.unfuse_lora()

    def unload_lora_weights(self):
        self.transformer.unload_lora()

    def delete_adapters(self, adapter_names):
        self.transformer.delete_adapters(adapter_names)

    def enable_lora(self):
        self.transformer.enable_adapters()

    def disable_lora(self):
        self.transformer.disable_adapters()

    # ------------------------------------------------------------------ IP-Adapter (image prompt): the FluxIPAdapterMixin subset, routed
    # to the transformer (ip_adapter.py); the image side is image_encoder.CLIPVisionModelWithProjection or SiglipVisionModel.
    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder: Optional[str] = None, weight_name: Optional[str] = None,
                        image_encoder_pretrained_model_name_or_path: Optional[str] = None, image_encoder_subfolder: Optional[str] = None,
                        **kwargs):
        """``image_encoder_pretrained_model_name_or_path`` (+ ``image_encoder_subfolder``): a local directory, or a hub id in the local
        hub cache, that holds a CLIP or SigLIP vision ``config.json`` (image_encoder.image_encoder_class picks the class) — loaded as
        ``self.image_encoder``. A name that does not resolve to one
        leaves the pipeline's encoder as it is (one log line): nothing is fetched, and ``ip_adapter_image_embeds`` need no encoder."""
        self.transformer.load_ip_adapter(pretrained_model_name_or_path_or_dict, subfolder=subfolder, weight_name=weight_name)
        name = image_encoder_pretrained_model_name_or_path
        if name is None:
            return
        from .modules import resolve_model_path

        try:
            d = resolve_model_path(name)
            d = os.path.join(d, image_encoder_subfolder) if image_encoder_subfolder else d
        except OSError:
            d = None
        if d is None or not os.path.isfile(os.path.join(d, "config.json")):
            import sys
            print(f"[reptext_amd] load_ip_adapter: image encoder '{name}' is not a local directory with a config.json; keeping "
                  f"image_encoder = {type(self.image_encoder).__name__}", file=sys.stderr, flush=True)
            return
        from .image_encoder import image_encoder_class

        enc = image_encoder_class(d).from_pretrained(d, torch_dtype=torch.bfloat16)
        self.image_encoder = enc.to(self.transformer.device)

    def set_ip_adapter_scale(self, scale):
        self.transformer.set_ip_adapter_scale(scale)

    def unload_ip_adapter(self):
        self.transformer.unload_ip_adapter()

    def _resolve_ip_embeds(self, ip_adapter_image, ip_adapter_image_embeds, joint_attention_kwargs, batch_size, num_images_per_prompt, device):
        """(embeds [total or 1, E] bf16 on the device, or None when the adapter has nothing to add; joint_attention_kwargs without the
        embeds). The embeds may also arrive as joint_attention_kwargs["ip_adapter_image_embeds"], where diffusers' pipeline puts them."""
        from . import ip_adapter as _ipa

        kw = joint_attention_kwargs
        if ip_adapter_image is not None:
            if ip_adapter_image_embeds is not None or (kw is not None and "ip_adapter_image_embeds" in kw):
                raise ValueError("pass either ip_adapter_image or ip_adapter_image_embeds, not both")
            if self.image_encoder is None:
                raise NotImplementedError("ip_adapter_image needs an image encoder, which this pipeline does not have: encode the image "
                                          "yourself and pass ip_adapter_image_embeds")
            if isinstance(ip_adapter_image, torch.Tensor):
                n = ip_adapter_image.shape[0] if ip_adapter_image.dim() == 4 else 1
            else:
                n = len(ip_adapter_image) if isinstance(ip_adapter_image, (list, tuple)) else 1
            if n not in (1, batch_size):
                raise ValueError(f"ip_adapter_image: {n} images for a batch of {batch_size} (one image per sample, or one for all)")
            ip_adapter_image_embeds = self.encode_image(ip_adapter_image, device)      # from here on as if the caller had passed them
        if kw is not None and "ip_adapter_image_embeds" in kw:
            if ip_adapter_image_embeds is not None:
                raise ValueError("ip_adapter_image_embeds were passed both as an argument and inside joint_attention_kwargs")
            ip_adapter_image_embeds = kw["ip_adapter_image_embeds"]
            kw = {k: v for k, v in kw.items() if k != "ip_adapter_image_embeds"} or None
        if ip_adapter_image_embeds is None:
            return None, kw
        adapter = getattr(self.transformer, "_ip_adapter", None)
        if adapter is None:
            raise ValueError("ip_adapter_image_embeds were passed but no IP-Adapter is loaded (load_ip_adapter)")
        e = _ipa.normalize_embeds(ip_adapter_image_embeds)
        total = batch_size * num_images_per_prompt
        if e.shape[0] == batch_size and total != batch_size:
            e = e.repeat_interleave(num_images_per_prompt, dim=0)
        if e.shape[0] not in (1, total):
            raise ValueError(f"ip_adapter_image_embeds: batch {e.shape[0]} is neither 1 nor the number of images {total}")
        if e.shape[1] != adapter.E:
            raise ValueError(f"ip_adapter_image_embeds: width {e.shape[1]} != the adapter's image embedding width {adapter.E}")
        if not adapter.active:
            return None, kw
        return e.to(device=device, dtype=torch.bfloat16).contiguous(), kw

    def encode_image(self, image, device=None, num_images_per_prompt: int = 1) -> torch.Tensor:
        """[B·num_images_per_prompt, E] bf16 image embeddings of ``self.image_encoder``: ``image_embeds`` of the CLIP encoder,
        ``pooler_output`` of a ``SiglipVisionModel``. A tensor is taken as ``pixel_values`` (diffusers' rule); anything else goes through
        ``self.feature_extractor(images=..., return_tensors="pt")`` when one is set, else ``image_encoder.clip_preprocess`` /
        ``siglip_preprocess`` at the encoder's image size. One encoder run on the current stream."""
        if self.image_encoder is None:
            raise ValueError("encode_image: this pipeline has no image_encoder")
        device = device or self._execution_device
        from .image_encoder import SiglipVisionModel

        siglip = isinstance(self.image_encoder, SiglipVisionModel)
        if isinstance(image, torch.Tensor):
            pixel_values = image if image.dim() == 4 else image[None]
        elif self.feature_extractor is not None:
            pixel_values = self.feature_extractor(images=image, return_tensors="pt").pixel_values
        else:
            from .image_encoder import clip_preprocess, siglip_preprocess

            pixel_values = (siglip_preprocess if siglip else clip_preprocess)(image, size=self.image_encoder.config.image_size)
        out = self.image_encoder(pixel_values.to(device))
        embeds = out.pooler_output if siglip else out.image_embeds
        return embeds.repeat_interleave(num_images_per_prompt, dim=0) if num_images_per_prompt != 1 else embeds

    def _lora_models(self) -> list:
        cn = self.controlnet
        nets = list(cn.nets) if isinstance(cn, FluxMultiControlNetModel) else [cn]
        models = [self.transformer] + nets + [getattr(self, "controlnet_inpaint", None), getattr(self, "controlnet_union", None)]
        return [m for m in models if m is not None and getattr(m, "_lora", None) is not None]

    def _apply_lora_scale(self) -> None:
        """PIPE:908-925: the call's joint_attention_kwargs["scale"] merged into every model that carries adapters, before the loop
        and on the current stream (the tower's side stream waits on it). The models' own per-call check then finds nothing to do."""
        for m in self._lora_models():
            m._apply_lora_scale(self.joint_attention_kwargs)

    def _graph_safe_kwargs(self) -> bool:
        """No joint_attention_kwargs, or only a LoRA "scale" while adapters are loaded: that one is in the weights already."""
        kw = self.joint_attention_kwargs
        return kw is None or (set(kw) == {"scale"} and bool(self._lora_models()))

    # ------------------------------------------------------------------ the second ControlNet (controlnet_union)
    def _check_union_inputs(self, image, height, width, total) -> bool:
        """Refusals of the call's ``control_image_union`` (``image``) against ``self.controlnet_union`` and the first tower — host-side
        checks on shapes and configs only, made before any device work. True when the union tower takes part in this call."""
        if image is None:
            return False
        un, cn = self.controlnet_union, self.controlnet
        if un is None:
            raise ValueError("control_image_union was passed but this pipeline has no second ControlNet: set pipe.controlnet_union")
        if not isinstance(cn, FluxControlNetModel):
            raise ValueError("control_image_union needs pipe.controlnet to be a FluxControlNetModel: the union tower adds into the first "
                             "tower's sample buffers (a union tower without a RepText tower is not supported)")
        if un.union:
            raise NotImplementedError("ControlNet-Union mode embedding is outside the RepText hot path (SURVEY.md §2 #11): "
                                      "controlnet_union must have num_mode=None (Union-Pro-2.0)")
        depth = lambda m: (len(m.transformer_blocks), len(m.single_transformer_blocks))
        if depth(un)[0] > depth(cn)[0] or depth(un)[1] > depth(cn)[1]:
            raise ValueError(f"control_image_union: controlnet_union has {depth(un)} double/single blocks, more than the first tower's "
                             f"{depth(cn)}: there is one sample buffer per block of the first tower")
        if un.inner_dim != cn.inner_dim:
            raise ValueError(f"control_image_union: controlnet_union's inner_dim {un.inner_dim} != the first tower's {cn.inner_dim}")
        if isinstance(image, torch.Tensor) and image.dim() == 3:          # packed hint latents [B, N, in_channels]
            width_in = un.controlnet_x_embedder.weight.shape[1]
            n_rows = (int(height) // self.vae_scale_factor) * (int(width) // self.vae_scale_factor)
            if image.shape[-1] != width_in:
                raise ValueError(f"control_image_union: packed hint width {image.shape[-1]} != controlnet_union's hint width {width_in}")
            if image.shape[0] not in (1, total):
                raise ValueError(f"control_image_union: packed hint batch {image.shape[0]} is neither 1 nor the number of images {total}")
            if image.shape[1] != n_rows:
                raise ValueError(f"control_image_union: packed hint has N = {image.shape[1]} rows, {height}x{width} pixels need {n_rows}")
        elif self.vae is None:
            raise ValueError("control_image_union: an image needs the pipeline's VAE; pass packed [B, N, 64] hint latents instead")
        return True

    def _union_hint(self, image, width, height, total, num_images_per_prompt, device, dtype) -> torch.Tensor:
        """[B or 1, N, 64] hint of the union tower: packed latents as they are, an image as ``prepare_image`` treats the canny hint
        (preprocess, VAE posterior SAMPLE from the global RNG (Q2), (z - shift)·scale, pack) without the position channels."""
        if self._is_packed_hint(image, self.controlnet_union):
            return image.to(device=device, dtype=dtype)
        image = self._prep_pixels(image, width, height, total, num_images_per_prompt, device, dtype)
        sf, sc = self.vae.config.shift_factor, self.vae.config.scaling_factor
        lat = ((self.vae.encode(image.to(self.vae.dtype)).latent_dist.sample() - sf) * sc).to(dtype)
        return self._pack_latents(lat, lat.shape[0], lat.shape[1], lat.shape[2], lat.shape[3])

    # ------------------------------------------------------------------ the negative prompt (true CFG)
    def _check_true_cfg_inputs(self, a: CallExtensions, prompt_embeds, pooled_prompt_embeds, batch_size, joint_attention_kwargs) -> bool:
        """Refusals of the negative-prompt arguments in ``a`` — host-side checks on types and shapes only, made before any device work
        and whether or not the scale switches CFG on. True when this call runs true CFG (``do_true_cfg``); a scale above 1 without a
        negative prompt logs one line and is the plain call."""
        neg, neg2 = a.negative_prompt, a.negative_prompt_2
        npe, npooled = a.negative_prompt_embeds, a.negative_pooled_prompt_embeds
        if (npe is None) != (npooled is None):
            missing = "negative_pooled_prompt_embeds" if npooled is None else "negative_prompt_embeds"
            raise ValueError(f"`{missing}` is missing: negative_prompt_embeds and negative_pooled_prompt_embeds have to be passed together")
        for name, value in (("negative_prompt", neg), ("negative_prompt_2", neg2)):
            if value is not None and npe is not None:
                raise ValueError(f"Cannot forward both `{name}` and `negative_prompt_embeds`. Please make sure to only forward one of the two.")
            if value is not None and not isinstance(value, (str, list)):
                raise ValueError(f"`{name}` has to be of type `str` or `list` but is {type(value)}")
            if isinstance(value, list) and len(value) != batch_size:
                raise ValueError(f"`{name}`: {len(value)} negative prompts for a batch of {batch_size} prompts (one per prompt, or one string for all)")
        if npe is not None and prompt_embeds is not None:
            self._check_negative_embeds_shape(npe, npooled, prompt_embeds, pooled_prompt_embeds)
        kw = joint_attention_kwargs or {}
        positive_ip = a.ip_adapter_image is not None or a.ip_adapter_image_embeds is not None or "ip_adapter_image_embeds" in kw
        for name in ("negative_ip_adapter_image", "negative_ip_adapter_image_embeds"):
            if getattr(a, name) is not None and not positive_ip:
                raise ValueError(f"`{name}` was passed without a positive image prompt (ip_adapter_image / ip_adapter_image_embeds)")
        if a.negative_ip_adapter_image is not None and a.negative_ip_adapter_image_embeds is not None:
            raise ValueError("pass either negative_ip_adapter_image or negative_ip_adapter_image_embeds, not both")
        on = do_true_cfg(a.true_cfg_scale, neg, npe, npooled)
        if not on and float(a.true_cfg_scale) > 1:
            import sys
            print(f"[reptext_amd] true_cfg_scale = {a.true_cfg_scale} without a negative prompt: classifier-free guidance stays off",
                  file=sys.stderr, flush=True)
        return on

    @staticmethod
    def _check_negative_embeds_shape(npe, npooled, prompt_embeds, pooled_prompt_embeds) -> None:
        if tuple(npe.shape) != tuple(prompt_embeds.shape):
            raise ValueError(f"`negative_prompt_embeds`: shape {tuple(npe.shape)} != prompt_embeds' {tuple(prompt_embeds.shape)}")
        if tuple(npooled.shape) != tuple(pooled_prompt_embeds.shape):
            raise ValueError(f"`negative_pooled_prompt_embeds`: shape {tuple(npooled.shape)} != pooled_prompt_embeds' "
                             f"{tuple(pooled_prompt_embeds.shape)}")

    def _encode_negative_prompt(self, a: CallExtensions, prompt_embeds, pooled_prompt_embeds, batch_size, num_images_per_prompt,
                                max_sequence_length, device):
        """(negative prompt_embeds, negative pooled) of the call ``a``, shaped like the positive ones: the embeddings as passed, or the
        negative prompt through ``encode_prompt`` (``negative_prompt_2`` defaults to ``negative_prompt``; one string serves the batch)."""
        npe, npooled = a.negative_prompt_embeds, a.negative_pooled_prompt_embeds
        if npe is None:
            per_prompt = lambda p: [p] * batch_size if isinstance(p, str) else p
            neg = per_prompt(a.negative_prompt)
            neg2 = per_prompt(a.negative_prompt_2) if a.negative_prompt_2 is not None else neg
            npe, npooled, _ = self.encode_prompt(prompt=neg, prompt_2=neg2, device=device, num_images_per_prompt=num_images_per_prompt,
                                                 max_sequence_length=max_sequence_length)
        self._check_negative_embeds_shape(npe, npooled, prompt_embeds, pooled_prompt_embeds)
        return npe.to(device=device, dtype=prompt_embeds.dtype), npooled.to(device=device, dtype=pooled_prompt_embeds.dtype)

    def _negative_ip_embeds(self, a: CallExtensions, positive: torch.Tensor, total: int, device) -> torch.Tensor:
        """The image prompt of the negative half, shaped like ``positive`` ([total or 1, E], what ``_resolve_ip_embeds`` returned):
        ``negative_ip_adapter_image_embeds`` if given, else ``negative_ip_adapter_image`` through ``encode_image``, else an all-black
        image through the same encoder when the positive one was an image, else a zero embedding."""
        from . import ip_adapter as _ipa

        neg_image, neg_embeds = a.negative_ip_adapter_image, a.negative_ip_adapter_image_embeds
        if neg_embeds is None and neg_image is None and a.ip_adapter_image is not None:
            if self.image_encoder is not None:
                neg_image = self._black_image(self.image_encoder.config.image_size)
        if neg_embeds is None and neg_image is not None:
            if self.image_encoder is None:
                raise NotImplementedError("negative_ip_adapter_image needs an image encoder, which this pipeline does not have: encode the "
                                          "image yourself and pass negative_ip_adapter_image_embeds")
            neg_embeds = self.encode_image(neg_image, device)
        if neg_embeds is None:
            return torch.zeros_like(positive)
        e = _ipa.normalize_embeds(neg_embeds).to(device=device, dtype=torch.bfloat16)
        if e.shape[1] != positive.shape[1]:
            raise ValueError(f"negative_ip_adapter_image_embeds: width {e.shape[1]} != the adapter's image embedding width {positive.shape[1]}")
        if e.shape[0] not in (1, positive.shape[0]):
            raise ValueError(f"negative_ip_adapter_image_embeds: batch {e.shape[0]} is neither 1 nor the positive image prompt's {positive.shape[0]}")
        return e.expand(positive.shape[0], -1)

    @staticmethod
    def _black_image(size: int):
        """The default negative image prompt: an all-black PIL image, preprocessed and encoded like any other."""
        from PIL import Image

        return Image.new("RGB", (size, size), (0, 0, 0))

    # ------------------------------------------------------------------ the call
    @accepts_call_extensions(*PerturbedCallExtensions.__dataclass_fields__)
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]] = None, prompt_2: Optional[Union[str, List[str]]] = None,
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 28,
                 timesteps: List[int] = None, guidance_scale: float = 7.0,
                 control_guidance_start: Union[float, List[float]] = 0.0, control_guidance_end: Union[float, List[float]] = 1.0,
                 control_image: PipelineImageInput = None, control_mode: Optional[Union[int, List[int]]] = None,
                 controlnet_conditioning_scale: Union[float, List[float]] = 1.0, controlnet_conditioning_step: int = 30,
                 num_images_per_prompt: Optional[int] = 1,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                 latents: Optional[torch.FloatTensor] = None, prompt_embeds: Optional[torch.FloatTensor] = None,
                 pooled_prompt_embeds: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, joint_attention_kwargs: Optional[Dict[str, Any]] = None,
                 callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 512,
                 control_mask: Optional[torch.FloatTensor] = None, control_position: Optional[torch.FloatTensor] = None,
                 control_glyph: Optional[torch.FloatTensor] = None):
        return self._generate(None, prompt, prompt_2, height, width, num_inference_steps, timesteps, guidance_scale, control_guidance_start,
                              control_guidance_end, control_image, control_mode, controlnet_conditioning_scale, controlnet_conditioning_step,
                              num_images_per_prompt, generator, latents, prompt_embeds, pooled_prompt_embeds, output_type, return_dict,
                              joint_attention_kwargs, callback_on_step_end, callback_on_step_end_tensor_inputs, max_sequence_length,
                              control_mask, control_position, control_glyph)

    def _generate(self, start, prompt, prompt_2, height, width, num_inference_steps, timesteps, guidance_scale, control_guidance_start,
                  control_guidance_end, control_image, control_mode, controlnet_conditioning_scale, controlnet_conditioning_step,
                  num_images_per_prompt, generator, latents, prompt_embeds, pooled_prompt_embeds, output_type, return_dict,
                  joint_attention_kwargs, callback_on_step_end, callback_on_step_end_tensor_inputs, max_sequence_length, control_mask,
                  control_position, control_glyph):
        """The body of ``__call__``, whose arguments these are, in its order. ``start`` is whatever a subclass's ``__call__`` wants its own
        ``_cut_schedule`` and ``_start_state`` to receive (a value of one call, so that nothing of it lives on the pipeline); None here."""
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        # control_guidance_start/end are normalised like the reference but have no effect on the result (inert: Q3)
        self.check_inputs(prompt, prompt_2, height, width, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                          callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, max_sequence_length=max_sequence_length)
        self._guidance_scale, self._joint_attention_kwargs, self._interrupt = guidance_scale, joint_attention_kwargs, False
        batch_size = self._batch_size(prompt, prompt_embeds)
        device, dtype = self._execution_device, self.transformer.dtype
        total = batch_size * num_images_per_prompt
        ext = self._call_extensions
        with_union = self._check_union_inputs(ext.control_image_union, height, width, total)
        cfg = self._check_true_cfg_inputs(ext, prompt_embeds, pooled_prompt_embeds, batch_size, joint_attention_kwargs)
        # perturbed-attention guidance: prepared as a true-CFG call whose first half is the positive conditioning itself (``Perturbed``)
        pag = pag_arguments(ext, self.transformer, cfg)
        true_cfg, cfg = cfg, cfg or pag is not None
        line_entries = line_prompt_arguments(ext, len(control_image) if control_image is not None else 0, control_mask,
                                             bool(getattr(self.transformer, "_fp8_attention", False)))
        isolation = line_isolation_argument(ext, line_entries)
        line_scales = line_scale_argument(ext, line_entries, len(control_image) if control_image is not None else 0)
        positive_ip = (ext.ip_adapter_image is not None or ext.ip_adapter_image_embeds is not None
                       or "ip_adapter_image_embeds" in (joint_attention_kwargs or {}))
        regional_args = regional_ip_arguments(ext, len(control_image) if control_image is not None else 0, control_mask,
                                              getattr(self.transformer, "_ip_adapter", None), positive_ip, self.image_encoder is not None)
        ip_embeds, self._joint_attention_kwargs = self._resolve_ip_embeds(ext.ip_adapter_image, ext.ip_adapter_image_embeds, joint_attention_kwargs,
                                                                          batch_size, num_images_per_prompt, device)
        if cfg and ip_embeds is not None:
            # [2·total, E], negative first like the prompt: rt_ip_attention takes K/V per entry of the conditioning batch
            pos = ip_embeds.expand(total, -1)
            ip_embeds = torch.cat([self._negative_ip_embeds(ext, pos, total, device) if true_cfg else pos, pos], dim=0).contiguous()

        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds, device=device,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        prompt_embeds = prompt_embeds.to(device=device)
        pooled_prompt_embeds = pooled_prompt_embeds.to(device=device)
        if cfg:
            # True CFG: the conditioning batch is cat([negative, positive]) (negative first, INP:1034-1035) against latents of batch B;
            # the models repeat the latents over it, and the step mixes the two halves of the velocity (LoopExtras.cfg_scale)
            npe, npooled = self._encode_negative_prompt(ext, prompt_embeds, pooled_prompt_embeds, batch_size, num_images_per_prompt,
                                                        max_sequence_length, device) if true_cfg else (prompt_embeds, pooled_prompt_embeds)
            prompt_embeds = torch.cat([npe, prompt_embeds], dim=0)
            pooled_prompt_embeds = torch.cat([npooled, pooled_prompt_embeds], dim=0)

        hints, height, width = self._collect_hints(control_image, control_position, height, width, total, num_images_per_prompt, device, dtype,
                                                   cfg=cfg)
        # the union hint is encoded AFTER the text lines' hints: a call without it draws the same random numbers as before
        union_hint = self._doubled_under_cfg(self._union_hint(ext.control_image_union, width, height, total, num_images_per_prompt, device, dtype),
                                             total, cfg) if with_union else None
        timesteps, num_inference_steps = self._schedule(height, width, num_inference_steps, timesteps, device)
        timesteps, num_inference_steps = self._cut_schedule(start, timesteps, num_inference_steps)
        latents, latent_image_ids, repaint = self._start_state(start, control_glyph, total, height, width, prompt_embeds.dtype, device, generator, latents)
        region = self._region_masks(control_mask, latents.device, prompt_embeds.dtype)
        masks = [self._doubled_under_cfg(m, total, cfg, mask=True) for m in region]
        line_prompts = self._line_prompts(line_entries, ext, region, prompt_embeds, latents.shape[1], total, num_images_per_prompt, cfg, device,
                                          isolation)
        active = union_active_steps(len(timesteps), float(ext.control_guidance_start_union), float(ext.control_guidance_end_union)) if with_union else ()
        union = UnionTower(self.controlnet_union, union_hint, float(ext.controlnet_conditioning_scale_union), active) if active else None
        regional = self._regional_ip(regional_args, ip_embeds, region, latents.shape[1], total, num_images_per_prompt, cfg, device,
                                     prompt_embeds.dtype)
        perturbed = None
        if pag is not None:
            row_vis, key_class = perturbed_attention_tables(prompt_embeds.shape[1], latents.shape[1], total)
            perturbed = Perturbed(row_vis.to(device), key_class.to(device), pag[1], pag[2])
        cfg_scale = (float(ext.true_cfg_scale) if true_cfg else pag[0]) if cfg else None
        # stochastic sampling: the samples' noise streams, named by the call's generator after the start state has drawn from it (without
        # the switch nothing is built and nothing is drawn)
        step_noise = StepNoise(stochastic_rng(generator, latents.shape[0]).to(device)) if getattr(self.scheduler, "stochastic_sampling", False) else None
        extras = LoopExtras(ip_embeds=ip_embeds if regional is None else None, union=union, cfg_scale=cfg_scale,
                            repaint=repaint, guidance=loop_guidance(self.guider, cfg, len(timesteps)), line_prompts=line_prompts,
                            regional_ip=regional,
                            line_scale=None if line_scales is None else LineScale(
                                line_prompt_bias(line_scales, [e is not None for e in line_entries]).to(device)),
                            perturbed=perturbed, step_noise=step_noise)

        self._apply_lora_scale()
        latents = self._denoise(latents, prompt_embeds, pooled_prompt_embeds, text_ids, latent_image_ids, timesteps, hints, masks,
                                guidance_scale, controlnet_conditioning_scale, controlnet_conditioning_step, control_mode,
                                callback_on_step_end, callback_on_step_end_tensor_inputs, num_inference_steps, extras)
        return self._finish(latents, height, width, output_type, return_dict)

    def _regional_ip(self, args, ip_embeds, region, N, total, num_images_per_prompt, cfg, device, dtype) -> Optional[RegionalIP]:
        """The call's image prompts as ordered, weighted terms (None: no table and no line term, the loop takes ``ip_embeds`` as it always
        did). ``args``: what ``regional_ip_arguments`` returned; ``ip_embeds``: the call's own prompt as the loop would take it (under true
        CFG [negative, positive]); ``region``: the text lines' resized masks. The weights are ``ip_adapter.regional_ip_weights``'s."""
        from . import ip_adapter as _ipa

        if args is None or not self.transformer._ip_adapter.active:
            return None
        entries, scales, mask = args
        embeds, img_w, txt_w = [], [], []
        if ip_embeds is not None:
            m = None if mask is None else self._region_masks([mask], device, dtype)[0]
            if m is not None and m.shape[1] != N:
                raise ValueError(f"ip_adapter_mask: {m.shape[1]} tokens after the resize, the image has {N}")
            w = _ipa.regional_ip_weights(m, 1.0, N=N, batch=total, cfg=cfg)
            embeds.append(ip_embeds), img_w.append(w[0]), txt_w.append(w[1])
        lines = [i for i, e in enumerate(entries) if e is not None]
        images = [entries[i] for i in lines if not (isinstance(entries[i], torch.Tensor) and entries[i].dim() == 2)]
        if images:      # every line's image in one encoder batch
            if all(isinstance(im, torch.Tensor) for im in images):
                images = torch.cat([im if im.dim() == 4 else im[None] for im in images])
            encoded = iter(self.encode_image(images, device).split(1))
        for i in lines:
            e = entries[i] if isinstance(entries[i], torch.Tensor) and entries[i].dim() == 2 else next(encoded)
            if e.shape[0] == total // num_images_per_prompt and num_images_per_prompt != 1:
                e = e.repeat_interleave(num_images_per_prompt, dim=0)
            if e.shape[0] not in (1, total):
                raise ValueError(f"a text line's image prompt has batch {e.shape[0]}, neither 1 nor the number of images {total}")
            e = e.to(device=device, dtype=torch.bfloat16)
            w = _ipa.regional_ip_weights(region[i], scales[i], N=N, batch=total, cfg=cfg, line=True)
            embeds.append((torch.cat([e, e]) if cfg and e.shape[0] != 1 else e).contiguous()), img_w.append(w[0]), txt_w.append(w[1])
        if not lines and (not embeds or img_w[0] is None):
            return None
        dev = lambda t: None if t is None else t.to(device)
        return RegionalIP(tuple(embeds), tuple(dev(w) for w in img_w), tuple(dev(w) for w in txt_w))

    def _line_prompts(self, entries, ext, region, prompt_embeds, N, total, num_images_per_prompt, cfg, device,
                      isolation: bool = False) -> Optional[LinePrompts]:
        """The call's per-line prompts as the loop takes them (None: the call has none). T5 only: the pooled CLIP vector stays the base
        prompt's. Under true CFG the line embeddings serve both halves; the negative half's image rows do not see them."""
        if entries is None:
            return None
        L, Bc, T0 = ext.control_prompt_max_sequence_length, prompt_embeds.shape[0], prompt_embeds.shape[1]
        has_prompt = [e is not None for e in entries]
        # with isolation only the group ENDS (the text layout, and the rule's own refusals) are taken from it; the row table is line_prompt_classes'
        ends, row_vis = line_prompt_groups(T0, L, region, N, has_prompt, batch=total, cfg=cfg)
        embeds = []
        for e in entries:
            if isinstance(e, str):
                self._require_text_stack()
                e = self._get_t5_prompt_embeds([e] * (total // num_images_per_prompt), num_images_per_prompt, L, device)
            elif e is not None:
                if e.shape[0] not in (1, total // num_images_per_prompt) or e.shape[2] != prompt_embeds.shape[2]:
                    raise ValueError(f"control_prompt_embeds: an entry is [B or 1, {L}, {prompt_embeds.shape[2]}] with B the prompt's batch, got {tuple(e.shape)}")
                e = e.expand(total // num_images_per_prompt, -1, -1).repeat_interleave(num_images_per_prompt, dim=0)
            if e is not None:
                e = e.to(device=device, dtype=prompt_embeds.dtype)
                embeds.append(torch.cat([e, e]) if cfg else e)
        assert all(e.shape[0] == Bc for e in embeds)
        if isolation:
            row_vis, key_class = line_prompt_classes(T0, L, region, N, has_prompt, batch=total, cfg=cfg)
            return IsolatedLinePrompts(torch.cat(embeds, dim=1).contiguous(), ends, row_vis.to(device), key_class.to(device))
        return LinePrompts(torch.cat(embeds, dim=1).contiguous(), ends, row_vis.to(device))

    # ------------------------------------------------------------------ stages of the call (shared with pipeline_inpaint.py)
    @staticmethod
    def _batch_size(prompt, prompt_embeds) -> int:
        if isinstance(prompt, str):
            return 1
        return len(prompt) if isinstance(prompt, list) else prompt_embeds.shape[0]

    @staticmethod
    def _doubled_under_cfg(t: torch.Tensor, total: int, cfg: bool, mask: bool = False) -> torch.Tensor:
        """Under CFG the conditioning batch is [negative, positive]: a per-image tensor ([total,N,·]) is doubled, a shared one ([1,N,·])
        serves both halves. At ``total == 1`` the two forms coincide: a hint counts as per-image, a ``mask`` ([1,N,1], the reference's
        form) as shared."""
        per_image = t.shape[0] == total and not (mask and total == 1)
        return torch.cat([t] * 2) if cfg and per_image else t

    def _collect_hints(self, control_image, control_position, height, width, total, num_images_per_prompt, device, dtype, cfg=False):
        """One packed [B,N,128] hint per text line (PIPE:928-942), doubled under true CFG; returns (hints, height, width) as
        ``prepare_image`` leaves the size. Tensors that are already packed hint latents ([B,N,in+extra]) are taken as they are —
        an extension used by the benchmarks and the multi-GPU broadcast. Only a single ``FluxControlNetModel`` is fed."""
        hints: List[torch.Tensor] = []
        if isinstance(self.controlnet, FluxControlNetModel) and control_image is not None:
            positions = control_position if control_position is not None else [None] * len(control_image)
            for img, pos in zip(control_image, positions):
                if self._is_packed_hint(img):
                    hints.append(self._doubled_under_cfg(img.to(device=device, dtype=dtype), total, cfg))
                else:
                    h, height, width = self.prepare_image(image=img, image_position=pos, width=width, height=height, batch_size=total,
                                                          num_images_per_prompt=num_images_per_prompt, device=device, dtype=dtype,
                                                          do_classifier_free_guidance=cfg)
                    hints.append(h)
        return hints, height, width

    def _schedule(self, height, width, num_inference_steps, timesteps, device):
        """Linear sigmas shifted by the resolution's mu (PIPE:960-981) -> (timesteps, number of steps)."""
        sigmas = np.linspace(1.0, 1 / num_inference_steps, num_inference_steps)
        image_seq_len = (int(height) // self.vae_scale_factor) * (int(width) // self.vae_scale_factor)
        sc = self.scheduler.config
        mu = calculate_shift(image_seq_len, sc.base_image_seq_len, sc.max_image_seq_len, sc.base_shift, sc.max_shift)
        timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps, sigmas, mu=mu)
        self._num_timesteps = len(timesteps)
        return timesteps, num_inference_steps

    def _cut_schedule(self, start, timesteps, num_inference_steps):
        """The steps of the grid that the loop runs: all of them (the repaint pipeline runs the last ``strength`` of them)."""
        return timesteps, num_inference_steps

    def _start_state(self, start, control_glyph, total, height, width, dtype, device, generator, latents):
        """(the loop's start state, image ids, the loop's ``Repaint`` record or None): the initial latents and no record."""
        return (*self._initial_latents(control_glyph, total, height, width, dtype, device, generator, latents), None)

    def _initial_latents(self, control_glyph, total, height, width, dtype, device, generator, latents):
        """(packed latents, image ids): from the glyph image when one is given (``latents`` is then ignored, as in the reference)."""
        num_channels_latents = self.transformer.config.in_channels // 4
        if control_glyph is None:
            return self.prepare_latents(total, num_channels_latents, height, width, dtype, device, generator, latents)
        init_image = self.image_processor.preprocess(control_glyph, height=height, width=width).to(dtype=torch.float32)
        return self.prepare_latents_reptext(init_image, total, num_channels_latents, height, width, dtype, device, generator, None)

    def _finish(self, latents, height, width, output_type, return_dict):
        if output_type == "latent":
            # The parity tap (PIPE:1132-1133). The loop's state is kept in fp32 (A.6: the scheduler steps in fp32), and that state
            # is what is returned: rounding it to bf16 here would by itself cost 1.8e-3 rel-L2, twice the whole loop's error.
            # `.to(torch.bfloat16)` gives the reference's bf16-run dtype.
            image = self._master_latents
        else:
            h2 = 2 * (int(height) // self.vae_scale_factor)
            w2 = 2 * (int(width) // self.vae_scale_factor)
            if output_type in ("pil", "np"):
                u8 = self.vae.decode_packed(latents, h2, w2, output_u8=True)
                image = self.image_processor.postprocess_u8(u8, output_type)
            elif output_type == "pt":
                image = (self.vae.decode_packed(latents, h2, w2) / 2 + 0.5).clamp(0, 1)
            else:
                raise ValueError(f"unsupported output_type {output_type}")
        self.maybe_free_model_hooks()
        if not return_dict:
            return (image,)
        return FluxPipelineOutput(images=image)

    reference_bf16_scalars = False     # True: round t, t/1000 and guidance to bf16 where the reference's bf16 run does (mmdit.py)

    def _model_timestep(self, t: float) -> float:
        """The value the models receive as `timestep` (PIPE:1025,1048: t.to(dtype) / 1000). fp32-exact by default; under
        `reference_bf16_scalars` the bf16 run's value bf16(bf16(t) / 1000)."""
        from . import mmdit

        mmdit.reference_bf16_scalars(self.reference_bf16_scalars)
        if not self.reference_bf16_scalars:
            return t / 1000.0
        return float((torch.tensor(t, dtype=torch.float32).to(torch.bfloat16) / 1000).to(torch.float32))

    # ------------------------------------------------------------------ hot loop (PIPE:1016-1130)
    def _denoise(self, latents, prompt_embeds, pooled, text_ids, image_ids, timesteps, hints, masks, guidance_scale,
                 cn_scale, cn_steps, control_mode, callback, callback_inputs, num_inference_steps, extras: Optional[LoopExtras] = None):
        """Eager loop, or the replay of its captured hipGraph when this exact call signature has been seen before (GRAPH_CAPTURE).
        ``extras``: what the call adds to the plain loop (None: nothing); under true CFG prompt_embeds / pooled / hints hold [negative, positive]."""
        tvals = timesteps.to(torch.float32).cpu().tolist()                 # host copies: no per-step device sync
        # the rows the regional masks leave non-zero: read here, never inside the loop or a capture; part of the call signature below
        win = active_row_window(masks, latents.shape[1]) if masks and len(masks) == len(hints) else None
        extras = replace(extras or LoopExtras(), tower_window=win)
        base = dict(latents=latents, prompt_embeds=prompt_embeds, pooled=pooled, text_ids=text_ids, image_ids=image_ids, hints=hints, masks=masks)

        def loop(named, extras, callback=None):              # the eager loop on ``base``, or on a graph's clones under the same names
            lat, pe, pool, tids, iids, hs, ms = (named[name] for name in base)
            return self._denoise_eager(lat, pe, pool, tids, iids, tvals, hs, ms, guidance_scale, cn_scale, cn_steps, control_mode,
                                       callback, callback_inputs, num_inference_steps, timesteps, extras=extras)

        if not (GRAPH_CAPTURE and getattr(self, "capture_graphs", True) and callback is None and latents.is_cuda
                and not self.interrupt and isinstance(self.controlnet, (FluxControlNetModel, type(None)))
                and (control_mode is None) and self._graph_safe_kwargs()):         # no graph for this call
            return loop(base, extras, callback)
        key, ins = self._graph_signature(base, extras, tvals, guidance_scale, cn_scale, cn_steps, num_inference_steps)
        cache = self.__dict__.setdefault("_graph_cache", {})
        ent = cache.get(key)
        if ent is None:                                      # first sight of this signature: eager (and warm), remember it
            if len(cache) >= GRAPH_CACHE_MAX:
                cache.pop(next(iter(cache)))
            cache[key] = "seen"
        elif ent == "seen":                                  # second call: capture
            ent = cache[key] = self._capture_loop(ins, extras, loop)
        if not isinstance(ent, dict):                        # "seen" just now, or "failed" (now or earlier)
            return loop(base, extras)
        return self._replay_loop(ent, ins, len(tvals), num_inference_steps)

    def _graph_signature(self, base, extras, tvals, guidance_scale, cn_scale, cn_steps, num_inference_steps):     # -> (key, static inputs by name)
        from . import mmdit as _mm
        _mm.reference_bf16_scalars(self.reference_bf16_scalars)      # the module switch follows THIS pipeline before the key is built
        sig = lambda t: (tuple(t.shape), str(t.dtype), tuple(t.stride()))
        ident = lambda m: (id(m), id(m._ensure_plans()), id(getattr(m, "_cx_pad", None)), bool(getattr(m, "_fp8_linears", False)),
                           bool(getattr(m, "_fp8_attention", False)))
        models = tuple(ident(m) for m in (self.transformer, self.controlnet) if m is not None)
        *single, hints, masks = base.values()
        key = (*(sig(t) for t in single), tuple(sig(h) for h in hints), tuple(sig(m) for m in masks),
               tuple(tvals), tuple(self.scheduler.sigmas.tolist()), float(guidance_scale), repr(cn_scale), int(cn_steps), int(num_inference_steps),
               str(base["latents"].device), models, bool(self.reference_bf16_scalars), bool(_mm.RESIDUAL_F32), bool(OVERLAP_TOWER), bool(_mm.FUSED_QK_ROPE),
               extras.tower_window, bool(TOWER_WINDOW))
        key += extras.signature(sig, ident, getattr(self.transformer, "_ip_adapter", None))
        if getattr(self.scheduler, "solver_order", 1) > 1:       # its weights are kernel scalars fixed by the sigmas and timesteps in the key
            key += (("solver", self.scheduler.solver_order),)
        if extras.step_noise is not None:       # eta is a kernel scalar, like the step index each node bakes; the seeds are a static input
            key += (("stochastic", self.scheduler.stochastic_eta),)
        return key, dict(base, hints=list(hints), masks=list(masks), **extras.tensors())

    def _capture_loop(self, ins, extras, loop):          # on clones of ``ins`` -> the graph's cache entry, or "failed": an optimisation, never a requirement
        from . import mmdit as _mm
        static = {name: [t.clone() for t in v] if isinstance(v, list) else v.clone() for name, v in ins.items()}
        keep = [m._ensure_plans() for m in (self.transformer, self.controlnet) if m is not None] + [getattr(self.controlnet, "_cx_pad", None)]
        keep += extras.kept(self.transformer)
        graph = torch.cuda.CUDAGraph()
        host = {n: getattr(self.scheduler, n) for n in ("_step_index", "_history_len") if hasattr(self.scheduler, n)}      # a capture must not move it
        # The graph bakes in device pointers. Buffers from caches that may evict them later (workspaces, attention scratch, sample
        # buffers, rope tables) are recorded during the capture and OWNED by its entry (test_graphs_of_two_shapes_keep_their_buffers).
        attn_keys = set(ops._ATTN_WS)
        _mm.CAPTURE_KEEP = ops.CAPTURE_KEEP = keep
        try:
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):     # calls of OTHER threads (RCCL's watchdog) do not invalidate it
                out = loop(static, extras.rebound(static))
        except Exception as e:
            import sys
            print(f"[reptext_amd] hipGraph capture of the denoise loop failed ({type(e).__name__}: {e}); staying eager", file=sys.stderr, flush=True)
            ops.drop_attention_workspaces(set(ops._ATTN_WS) - attn_keys)     # their zero fill was recorded, never executed
            self._zero_samples_for(getattr(self, "_sample_cache", None), None)      # and so was a zero fill of the sample buffers: no promise
            torch.cuda.synchronize()
            return "failed"
        finally:
            _mm.CAPTURE_KEEP = ops.CAPTURE_KEEP = None
            for name, value in host.items():
                setattr(self.scheduler, name, value)
        samples = getattr(self, "_sample_cache", None)       # what the capture wrote into; "window": the rows its zero-linears were restricted to
        keep.append(samples)
        keep.extend(dict(m._rope_cache) for m in (self.transformer, self.controlnet, extras.union and extras.union.model)
                    if m is not None and hasattr(m, "_rope_cache"))
        return {"graph": graph, "static": static, "out": out, "out32": self._master_latents, "keep": keep, "samples": samples, "window": self._sample_promise}

    def _replay_loop(self, ent, ins, n_steps, num_inference_steps):      # refresh the entry's static inputs from ``ins`` and replay its graph
        tensors = lambda named: [t for v in named.values() for t in (v if isinstance(v, list) else [v])]
        for dst, src in zip(tensors(ent["static"]), tensors(ins)):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
        self._zero_samples_for(ent["samples"], ent["window"])       # another call may have left rows outside this window non-zero
        ent["graph"].replay()
        first = self.scheduler._step_index if self.scheduler._step_index is not None else (self.scheduler._begin_index or 0)
        self.scheduler._step_index = first + n_steps       # what the eager loop's step() calls leave: they start at the begin index, if one is set
        if getattr(self.scheduler, "solver_order", 1) > 1 and n_steps > 0:
            self.scheduler._history_len = 1                                    # the history (the graph's own) holds the last step's velocity
        self._master_latents = ent["out32"].clone()
        with self.progress_bar(total=num_inference_steps) as bar:
            bar.update(num_inference_steps)
        return ent["out"].clone()

    @staticmethod
    def _zero_samples_for(cache, window) -> None:
        """The tower sample buffers of ``cache`` (a ``_SampleCache``) must read zero outside ``window``, whose rows alone the zero-linears
        will write. They are zeroed once, when ``cache.window`` changes, not per step (None: no promise — the full path overwrites every
        row, and a call with a union tower, which writes every row at its steps, zeroes inside its own step sequence instead)."""
        if cache is None:
            return
        if window is not None and cache.window != window:
            for buf in cache.double:
                buf.zero_()
        cache.window = window

    def _denoise_eager(self, latents, prompt_embeds, pooled, text_ids, image_ids, tvals, hints, masks, guidance_scale,
                       cn_scale, cn_steps, control_mode, callback, callback_inputs, num_inference_steps, timesteps,
                       extras: LoopExtras = LoopExtras()):
        """The one loop over timesteps, for both pipelines. Every tower — text lines, ``extras.extra_towers``, ``extras.union`` — is a
        ``_Tower`` of one list, and each step walks its entry of ``tower_schedule``, which alone decides who runs when and in which order."""
        union, extra_towers = extras.union, extras.extra_towers
        device, B = latents.device, latents.shape[0]
        guidance = torch.full((B,), float(guidance_scale), device=device, dtype=torch.float32) if self.transformer.config.guidance_embeds else None
        # one regional mask per text line, shared by the batch ([1,N,1], the reference's form) or one per image ([B,N,1])
        rowscales = [m.to(torch.float32).reshape(-1).contiguous() if m.shape[0] == 1 else m.to(torch.float32).reshape(m.shape[0], -1).contiguous() for m in masks]
        num_warmup = max(len(timesteps) - num_inference_steps * self.scheduler.order, 0)
        # adaLN vectors of every block for every step, once per image (timesteps/guidance/pooled are loop-invariant inputs); under
        # true CFG the conditioning batch is 2B against the latents' B (Q6) and the tables take guidance at that batch
        model_ts = [self._model_timestep(t) for t in tvals]
        g_tab = guidance if guidance is None or pooled.shape[0] == B else guidance.repeat(pooled.shape[0] // B)
        tab_t = self.transformer.build_modulation_table(model_ts, g_tab, pooled)
        fused_cn = isinstance(self.controlnet, FluxControlNetModel) and len(hints) > 0
        # The towers of every step and every tower of this call, numbered as `tower_schedule` numbers them. The union tower's table holds
        # ITS active steps only; the text lines share one table over the steps below `cn_steps`, whose steps the extra towers follow.
        union_active = union.active_steps if union is not None and isinstance(self.controlnet, FluxControlNetModel) else ()
        steps = tower_schedule(len(tvals), cn_steps, len(hints) if fused_cn else 0, union_active, len(extra_towers))
        towers: List[_Tower] = []
        if union_active:
            towers.append(_Tower(union.model, union.hint, union.scale, None,
                                 union.model.build_modulation_table([model_ts[i] for i in union_active], g_tab, pooled), masked=False))
        if fused_cn and cn_steps > 0:
            ts_c = model_ts[: min(len(model_ts), cn_steps)]
            tab_c = self.controlnet.build_modulation_table(ts_c, g_tab, pooled)
            towers += [_Tower(self.controlnet, h, cn_scale, rowscales[line] if rowscales else None, tab_c, masked=True) for line, h in enumerate(hints)]
            towers += [_Tower(m, h, s, None, m.build_modulation_table(ts_c, g_tab, pooled), masked=False) for m, h, s in extra_towers]
        # Loop-invariant work, once per image instead of once per step (the prompt and the hint latents do not change inside the
        # loop): context_embedder(prompt) of every model, controlnet_x_embedder(hint) per tower. A callback that replaces
        # prompt_embeds invalidates them (recomputed below).
        # Per-line prompts: the transformer alone reads cat([base prompt, line prompts]) with text ids of that length (zeros, like the
        # base prompt's) and the key groups; every tower, and a callback, sees the base prompt.
        lp = extras.line_prompts
        joint_text = lambda pe: pe if lp is None else torch.cat([pe, lp.embeds.to(pe.dtype)], dim=1)
        text_ids_t = text_ids if lp is None else torch.zeros(prompt_embeds.shape[1] + lp.embeds.shape[1], 3, device=text_ids.device, dtype=text_ids.dtype)
        prompt_t = joint_text(prompt_embeds)
        # control_prompt_scale: the bias table goes with the key groups, [1, 32] for every batch entry (a guider's positive half needs no view)
        bias_kw = {} if extras.line_scale is None else dict(_key_bias=extras.line_scale.key_bias)
        # pag_scale: the tables go to the guided steps' forward at 2B; a guider's unguided step runs the positive half without any
        pag_kw = {} if extras.perturbed is None else dict(_perturbed=extras.perturbed)

        def prepare_static(pe):
            static_t = self.transformer.prepare_static(joint_text(pe))
            for tw in towers:
                tw.static = tw.model.prepare_static(pe, tw.hint)
            return static_t

        static_t = prepare_static(prompt_embeds)
        # the image prompt's tokens and every block's K/V of them: loop-invariant too (ip_adapter.py steps 1-2)
        ip_prep = self.transformer._ip_adapter.prepare(extras.ip_embeds) if extras.ip_embeds is not None else None
        rip = extras.regional_ip
        if rip is not None:        # regional terms: one projection for all of them, a list of views (the text rows are the transformer's)
            ip_prep = self.transformer._ip_adapter.prepare_terms(rip.embeds, list(zip(rip.img_w, rip.txt_w)), T=prompt_t.shape[1])
        # Which tower samples does the transformer read? Block i takes sample i // ceil(n_blocks / n_samples) (A.3): with 6
        # samples against 19 double blocks the sixth is never consumed (Q5), so its block and zero-linear are not evaluated.
        # A tower of another depth adds into the first tower's buffers (it must not be deeper: there is one buffer per block
        # of the first tower) and every block of every tower is then evaluated.
        blocks_needed, sample_buf, single_buf, need_d = None, None, None, 0
        if fused_cn or towers:
            cnet = self.controlnet
            n_cd, n_cs = len(cnet.transformer_blocks), len(cnet.single_transformer_blocks)
            n_td, n_ts = len(self.transformer.transformer_blocks), len(self.transformer.single_transformer_blocks)
            need_d = 0 if n_cd == 0 else (n_td - 1) // int(np.ceil(n_td / n_cd)) + 1      # the transformer reads (and waits for) samples < need_d
            need_s = 0 if n_cs == 0 or n_ts == 0 else (n_ts - 1) // int(np.ceil(n_ts / n_cs)) + 1
            if all((len(tw.model.transformer_blocks), len(tw.model.single_transformer_blocks)) == (n_cd, n_cs) for tw in towers):
                blocks_needed = (min(need_d, n_cd), min(need_s, n_cs))
            # sample buffers: allocated once per shape, written by the zero-linear epilogues every step (no per-step allocation)
            Bc, N_, d_ = prompt_embeds.shape[0], latents.shape[1], cnet.inner_dim
            key = (Bc, N_, d_, n_cd, n_cs, str(device))
            if getattr(self, "_sample_cache", None) is None or self._sample_cache.key != key:
                mk = lambda n: [torch.empty(Bc, N_, d_, device=device, dtype=torch.bfloat16) for _ in range(n)]
                self._sample_cache = _SampleCache(key, mk(n_cd), mk(n_cs))
            sample_buf, single_buf = self._sample_cache.double, self._sample_cache.single
        # Zero-linears and the last block of the masked towers on the masked rows only (controlnet.forward: _window). The extra towers
        # are unmasked and ADD to every row of the buffers, step after step, so with them every row must be overwritten first: full path.
        use_window = (TOWER_WINDOW and any(tw.masked for tw in towers) and not extra_towers and blocks_needed is not None
                      and blocks_needed[0] >= 1 and blocks_needed[1] == 0 and self.controlnet.supports_row_window())
        self._tower_window_used = window = extras.tower_window if use_window else None
        # A union step writes every row, so with a union tower the "rows outside the window read zero" promise is kept by the step
        # sequence itself: the buffers count as dirty from the start and after every union step, and the first text-only step that
        # follows zeroes them on the tower's stream (captured with the loop; one fill per transition of the union interval).
        dirty = any(not tw.masked for tw in towers)
        self._sample_promise = None if dirty else window
        if fused_cn or towers:
            self._zero_samples_for(self._sample_cache, self._sample_promise)
        # fp32 master copy of the latents between steps (the models read its bf16 copy): the scheduler computes in fp32 anyway
        # (A.6); not rounding the STATE 28 times keeps the loop close to the fp32 reference path. Callbacks see the bf16 copy.
        lat32 = latents.to(torch.float32).contiguous()
        latents = latents.to(torch.bfloat16).contiguous().clone()
        # a multistep scheduler's velocity of the step before, fp32 like the state and owned here; its first step does not read it
        hist = torch.empty_like(lat32) if getattr(self.scheduler, "solver_order", 1) > 1 else None
        # A guider (true CFG only). At its steps the loop is the CFG loop, with the projected step where the guider asks for it: the
        # guidance difference of the step before and the partial sums are fp32 buffers owned here, beside the state. At the other steps
        # there is no negative half to evaluate: the models run on the positive half at batch B, through views of what the call prepared
        # at 2B (``cat([negative, positive])``: the positive half is the contiguous slice [B:] of every conditioning tensor).
        gd = extras.guidance
        guided_at = None if gd is None else frozenset(gd.steps)
        proj = None
        if gd is not None and gd.guider.projected and gd.steps:
            proj = ProjectedStep(gd.guider.eta, gd.guider.norm_threshold, gd.guider.momentum, torch.empty_like(lat32),
                                 torch.empty(ops.guidance_partials_shape(B, lat32[0].numel()), device=device, dtype=torch.float32))
        # stochastic sampling: the scheduler's record of the call's noise streams; every step draws at its absolute step index
        stoch = None if extras.step_noise is None else self.scheduler.stochastic_step(extras.step_noise.rng)
        Bc = prompt_embeds.shape[0]
        pos_rows = slice(Bc - B, Bc)

        def positive_half(pe, st):
            """(prompt, pooled, transformer's static embeddings, towers, sample buffers, single buffers, image prompt, the transformer's
            text stream, its key groups) of the positive half."""
            pos = lambda t: t if t is None or t.shape[0] != Bc else t[Bc - B:]
            tws = [replace(tw, hint=pos(tw.hint), rowscale=tw.rowscale if tw.rowscale is None or tw.rowscale.dim() == 1 else pos(tw.rowscale),
                           static=replace(tw.static, ctx=pos(tw.static.ctx), hint=pos(tw.static.hint))) for tw in towers]
            ip_pos = lambda p: replace(p, kv=[(pos(k), pos(v)) for k, v in p.kv], tok=pos(p.tok), rows_img=pos(p.rows_img), rows_joint=pos(p.rows_joint))
            ip = ip_prep and ([ip_pos(p) for p in ip_prep] if isinstance(ip_prep, list) else ip_pos(ip_prep))
            lead = lambda bufs: None if bufs is None else [b[:B] for b in bufs]
            return (pos(pe), pos(pooled), replace(st, ctx=pos(st.ctx), hint=pos(st.hint)), tws, lead(sample_buf), lead(single_buf), ip,
                    pos(joint_text(pe)), lp and lp.groups(slice(Bc - B, Bc)))

        half = positive_half(prompt_embeds, static_t) if gd is not None and len(gd.steps) < len(tvals) else None
        # Tower ∥ transformer: within a step the tower's chain of kernels and the transformer's are independent except that
        # transformer block i consumes tower sample i // 4 (A.3). The tower therefore runs on a side stream into preallocated
        # sample buffers and the transformer waits, block by block, on the event of the sample it needs. At batch 1 most
        # launches fill only 27/32 of their last round of workgroups (216 GEMM tiles on 256 CUs, 864 attention workgroups on
        # 512 slots); two independent chains in flight fill some of those holes. Results are bitwise those of the serial order.
        # `not extra_towers`: the inpaint flow is serial by decision (its second tower has no side stream or "tower" workspace of its
        # own yet); an extra tower added to the BASE flow would switch the overlap off here too — extend this rule then, not the call.
        # The base flow's union tower shares the side stream and the "tower" workspace with the text towers: the towers of a step are
        # serial with each other, only the transformer runs beside them.
        overlap = (OVERLAP_TOWER and bool(towers) and not extra_towers and device.type == "cuda"
                   and len(self.controlnet.single_transformer_blocks) == 0)
        side = sample_ev = None
        if overlap:
            if getattr(self, "_side_stream", None) is None or self._side_stream.device != device:
                self._side_stream = torch.cuda.Stream(device=device)
            side = self._side_stream
            sample_ev = [torch.cuda.Event() for _ in range(len(self.controlnet.transformer_blocks))]
        with (_Progress(num_inference_steps, disable=True) if extras.quiet else self.progress_bar(total=num_inference_steps)) as bar:
            for i, t in enumerate(tvals):
                if self.interrupt:
                    continue
                timestep = torch.full((B,), self._model_timestep(t), device=device, dtype=torch.float32)      # PIPE:1025,1048 (Q4)
                # the conditioning this step sees: everything (under true CFG at 2B), or the positive half outside a guider's interval
                guided = guided_at is None or i in guided_at
                everything = (prompt_embeds, pooled, static_t, towers, sample_buf, single_buf, ip_prep, prompt_t, lp and lp.groups())
                c_pe, c_pooled, c_static, c_towers, c_samples, c_singles, c_ip, c_pe_t, c_groups = everything if guided else half
                rows = None if guided else pos_rows        # of the modulation tables, which hold 2B rows per step
                merged = merged_single = events = None
                if steps[i]:
                    if overlap:
                        side.wait_stream(torch.cuda.current_stream())    # latents of this step (and, at i = 0, tables and hints) are ready
                        events = sample_ev                               # recorded by the last tower, once the sums are complete
                    with torch.cuda.stream(side) if overlap else contextlib.nullcontext():
                        if any(not towers[k].masked for k, _ in steps[i]):
                            dirty = True
                        elif window is not None and dirty:           # text-only step after a union step (or the first one of the call)
                            for buf in sample_buf:
                                buf.zero_()
                            dirty = False
                        done_d = done_s = 0       # leading buffers already written in this step: the zero-linear epilogues add to those
                        for n, (k, pos) in enumerate(steps[i]):
                            tw = c_towers[k]
                            bs, ss = tw.model(
                                hidden_states=latents, controlnet_cond=tw.hint, controlnet_mode=control_mode, conditioning_scale=tw.scale,
                                timestep=timestep, guidance=guidance, pooled_projections=c_pooled, encoder_hidden_states=c_pe,
                                txt_ids=text_ids, img_ids=image_ids, joint_attention_kwargs=self.joint_attention_kwargs, return_dict=False,
                                _rowscale=tw.rowscale, _accumulate_into=c_samples, _accumulate_single_into=c_singles, _overwrite=(done_d, done_s),
                                _sample_events=events if n == len(steps[i]) - 1 else None,
                                _mods=tw.table.step(pos) if rows is None else tw.table.step(pos, rows), _static=tw.static,
                                _ws_tag="tower" if overlap else "", _blocks_needed=blocks_needed, _window=window if tw.masked else None)
                            done_d = max(done_d, sum(b is not None for b in bs or ()))
                            done_s = max(done_s, sum(b is not None for b in ss or ()))
                        if events is not None:
                            for ev in events[done_d:need_d]:   # the transformer waits on these; a shallower union tower alone left them
                                ev.record(torch.cuda.current_stream())
                    # buffers no tower of this step wrote are not injected (None), the block-to-sample map keeps the first tower's depth
                    merged = [b if j < done_d else None for j, b in enumerate(c_samples)] or None
                    merged_single = [b if j < done_s else None for j, b in enumerate(c_singles)] or None
                noise_pred = self.transformer(
                    hidden_states=latents, timestep=timestep, guidance=guidance, pooled_projections=c_pooled,
                    encoder_hidden_states=c_pe_t, controlnet_block_samples=merged, controlnet_single_block_samples=merged_single,
                    txt_ids=text_ids_t, img_ids=image_ids, joint_attention_kwargs=self.joint_attention_kwargs, return_dict=False,
                    _mods=tab_t.step(i) if rows is None else tab_t.step(i, rows), _sample_events=events, _static=c_static, _ip=c_ip,
                    **({} if c_groups is None else dict(_groups=c_groups, **bias_kw)), **(pag_kw if guided else {}))[0]
                if events is not None:
                    torch.cuda.current_stream().wait_stream(side)     # the tower has finished reading `latents` (its last sample is unused, Q5)
                if extras.velocity is not None:
                    noise_pred = extras.velocity(i, noise_pred)
                cfg = extras.cfg_scale is not None and guided  # then noise_pred is [negative, positive], B each
                pj = proj if cfg else None                     # this step's guidance difference goes where the one before is read from
                self.scheduler.step_master_(noise_pred[:B] if cfg else noise_pred, lat32, latents, v_text=noise_pred[B:] if cfg else None,
                                            s=extras.cfg_scale if cfg else None, repaint=extras.repaint, history=hist, projected=pj,
                                            **({} if stoch is None else dict(stochastic=stoch)))
                if pj is not None:
                    pj.first = False
                if callback is not None:
                    env = {"latents": latents, "prompt_embeds": prompt_embeds}
                    out = callback(self, i, timesteps[i], {k: env[k] for k in callback_inputs})
                    if "latents" in out:
                        latents = out.pop("latents").to(torch.bfloat16).contiguous()
                        lat32 = latents.to(torch.float32)
                        if hist is not None:
                            self.scheduler.reset_history()       # the velocity before belongs to the replaced state: first order next
                        if proj is not None:
                            proj.first = True                    # and so does the guidance difference: no momentum next
                    if "prompt_embeds" in out:                       # the loop-invariant embeddings are no longer valid
                        prompt_embeds = out.pop("prompt_embeds")
                        static_t, prompt_t = prepare_static(prompt_embeds), joint_text(prompt_embeds)
                        half = half and positive_half(prompt_embeds, static_t)
                if i == len(tvals) - 1 or ((i + 1) > num_warmup and (i + 1) % self.scheduler.order == 0):
                    bar.update()
        self._master_latents = lat32          # fp32 state of the loop; `latents` is its bf16 copy
        return latents
