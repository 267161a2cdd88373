"""FluxControlNetRepaintPipeline: render text into an image the caller already has, by latent-blend inpainting.

The loop starts from the source image noised to the sigma of step ``t_start``, runs only the last ``strength · n`` steps of the
text-to-image schedule, and after every step puts the source, re-noised to the next sigma, back where the mask is 0. It needs no
second ControlNet and no CFG doubling: a step costs what a text-to-image step costs, and the tokens outside the mask end as the
source's latents bit for bit. The rules (``image`` / ``mask_image`` / ``strength``, the ``t_start`` formula, ``scale_noise``) are
diffusers' ``FluxInpaintPipeline`` / ``FluxControlNetInpaintPipeline`` as recalled — the package is absent, parity is unpinned
(DESIGN.md §7). The reference has no such flow; it only keeps ``get_timesteps`` as dead code (PIPE:474-483).

This file holds what the flow adds to the base call: the three arguments, their refusals (made in ``__call__``, before any device work),
and overrides of the two stages at which ``FluxControlNetPipeline._generate`` is split for it: ``_cut_schedule`` (the steps that run) and
``_start_state`` (source and mask, then the noise, then the start state and the loop's ``Repaint`` record). The three arguments travel
from ``__call__`` to the stages as one ``RepaintArguments`` value. The step itself is one HIP kernel (rt_repaint_euler_step_f32).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from . import ops
from .image_processor import PipelineImageInput, VaeImageProcessor
from .pipeline import PerturbedCallExtensions, FluxControlNetPipeline, Repaint, accepts_call_extensions


def repaint_t_start(num_inference_steps: int, strength: float) -> int:
    """The first step, of ``num_inference_steps``, that a repaint at ``strength`` runs: ``int(max(n − min(n·strength, n), 0))``
    (diffusers' ``get_timesteps``, recalled). ``strength`` outside [0, 1], or one that leaves no step, is refused."""
    n, strength = int(num_inference_steps), float(strength)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
    t_start = int(max(n - min(n * strength, n), 0))
    if n - t_start < 1:
        raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline steps is "
                         f"{n - t_start} which is < 1 and not appropriate for this pipeline.")
    return t_start


def _count(x, packed: bool) -> int:
    """How many images ``x`` holds: a list's length, the batch of a [B, C, H, W] or ``packed`` [B, N, 64] tensor, else one."""
    if isinstance(x, torch.Tensor):
        return x.shape[0] if x.dim() == 4 or packed else 1
    return len(x) if isinstance(x, (list, tuple)) else 1


@dataclass(frozen=True)
class RepaintArguments:
    """What the repaint ``__call__`` takes beyond the base call, as passed: the ``start`` value that ``_generate`` hands to this class's
    ``_cut_schedule`` and ``_start_state``. It lives as long as the call, never on the pipeline."""
    image: Any
    mask_image: Any
    strength: float
    control_mask: Any


class FluxControlNetRepaintPipeline(FluxControlNetPipeline):
    def __init__(self, scheduler, vae, text_encoder, tokenizer, text_encoder_2, tokenizer_2, transformer, controlnet):
        super().__init__(scheduler, vae, text_encoder, tokenizer, text_encoder_2, tokenizer_2, transformer, controlnet)
        self.mask_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_resize=True, do_convert_grayscale=True,
                                                do_normalize=False, do_binarize=True)

    def _is_packed(self, t) -> bool:
        """A tensor [B, N, 64]: packed latents (source or mask), taken as they are — an extension, like packed hints."""
        return isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[-1] == self.transformer.config.in_channels

    def _latent_grid(self, height, width):
        return 2 * (int(height) // self.vae_scale_factor), 2 * (int(width) // self.vae_scale_factor)

    def _source_latents(self, image, height, width, device, generator) -> torch.Tensor:
        """fp32 packed source latents [n, N, 64]: preprocess, VAE posterior SAMPLE with ``generator``, (z − shift)·scale, pack."""
        if self._is_packed(image):
            return image.to(device=device, dtype=torch.float32)
        pixels = self.image_processor.preprocess(image, height=height, width=width).to(device=device, dtype=self.vae.dtype)
        lat = self._encode_vae_image(pixels, generator).to(torch.float32)
        return self._pack_latents(lat, lat.shape[0], lat.shape[1], lat.shape[2], lat.shape[3])

    @staticmethod
    def _union_of_masks(control_mask):
        """The pixel-wise maximum of the text lines' ``control_mask`` images: every line's box is repainted. ``control_mask`` is the
        base call's list, one image per line, all of one size; anything else needs a ``mask_image``."""
        if not isinstance(control_mask, (list, tuple)) or len(control_mask) == 0:
            raise ValueError("pass `mask_image`, or `control_mask` as a list of images whose union is then the mask: there is nothing to repaint")
        if any(isinstance(m, torch.Tensor) for m in control_mask):
            raise ValueError("`mask_image` is required when `control_mask` holds token masks (tensors), not images")
        arrays = [np.array(m.convert("L")) if isinstance(m, Image.Image) else np.asarray(m) for m in control_mask]
        if any(a.ndim != 2 or a.shape != arrays[0].shape for a in arrays):
            raise ValueError(f"`mask_image` is required when the `control_mask` images are not single-channel images of one size "
                             f"(got {[a.shape for a in arrays]})")
        return Image.fromarray(np.maximum.reduce(arrays))

    def _check_repaint_inputs(self, a: RepaintArguments, total: int, height: int, width: int, num_inference_steps: int) -> None:
        """Host-side refusals of the three arguments, before any device work."""
        repaint_t_start(num_inference_steps, a.strength)
        if a.image is None:
            raise ValueError("`image` (the source to repaint) is required")
        if a.mask_image is None:
            self._union_of_masks(a.control_mask)
        shape = ((int(height) // self.vae_scale_factor) * (int(width) // self.vae_scale_factor), self.transformer.config.in_channels)
        for name, value in (("image", a.image), ("mask_image", a.mask_image)):
            if self._is_packed(value) and tuple(value.shape[1:]) != shape:
                raise ValueError(f"`{name}`: packed latents of shape {tuple(value.shape)}, {height}x{width} pixels need [B, {shape[0]}, {shape[1]}]")
        n = _count(a.image, self._is_packed(a.image))
        if n < 1 or total % n:
            raise ValueError(f"Cannot duplicate `image` of batch size {n} to {total} images.")
        n_mask = _count(a.mask_image, self._is_packed(a.mask_image))
        if a.mask_image is not None and n_mask not in (1, total):
            raise ValueError(f"`mask_image`: batch {n_mask} is neither 1 nor the number of images {total}")
        if not self._is_packed(a.image) and self.vae is None:
            raise ValueError("`image`: an image needs the pipeline's VAE; pass packed [B, N, 64] source latents instead")

    def _cut_schedule(self, start: RepaintArguments, timesteps, num_inference_steps):
        """``timesteps[t_start:]`` of the base grid; the scheduler begins at ``t_start``. (``start`` None: the base class's ``__call__``
        on this pipeline, which stays the text-to-image call.)"""
        if start is None:
            return super()._cut_schedule(start, timesteps, num_inference_steps)
        t_start = repaint_t_start(len(timesteps), start.strength)
        self.scheduler.set_begin_index(t_start)
        self._num_timesteps = len(timesteps) - t_start
        return timesteps[t_start:], len(timesteps) - t_start

    def _start_state(self, start: RepaintArguments, control_glyph, total, height, width, dtype, device, generator, latents):
        """Source and mask are encoded first — after the hints, before the noise is drawn: the source's posterior sample is the first
        draw from ``generator`` — then what the base returns, which is the noise; the start state is the source noised to the first
        sigma that runs (``_cut_schedule`` left its index as the scheduler's begin index), everywhere, in fp32."""
        if start is None:
            return super()._start_state(start, control_glyph, total, height, width, dtype, device, generator, latents)
        src = self._source_latents(start.image, height, width, device, generator)
        src32 = src.repeat_interleave(total // src.shape[0], dim=0).contiguous()
        mask = self._pack_mask(start.mask_image if start.mask_image is not None else self._union_of_masks(start.control_mask), height, width, device)
        noise, image_ids, _ = super()._start_state(start, control_glyph, total, height, width, dtype, device, generator, latents)
        noise32 = noise.to(torch.float32).contiguous()
        if noise32.shape != src32.shape:
            raise ValueError(f"`latents` (the noise) of shape {tuple(noise32.shape)} against source latents of shape {tuple(src32.shape)}")
        sigma = float(self.scheduler.sigmas[self.scheduler._begin_index])
        return self.scheduler.scale_noise(src32, sigma, noise32), image_ids, Repaint(src32, noise32, mask)

    def _pack_mask(self, mask_image, height, width, device) -> torch.Tensor:
        """fp32 [n, N, 64], 1 = repaint: binarise at the pixel size, nearest-resize to the latent grid, one copy per latent channel,
        pack like the latents."""
        if self._is_packed(mask_image):
            return mask_image.to(device=device, dtype=torch.float32).contiguous()
        m = self.mask_processor.preprocess(mask_image, height=height, width=width).to(device=device, dtype=torch.float32)
        grid = self._latent_grid(height, width)
        m = ops.resize2d(m, size=grid, mode="nearest") if m.is_cuda else F.interpolate(m, size=grid)
        channels = self.transformer.config.in_channels // 4
        return self._pack_latents(m.repeat(1, channels, 1, 1), m.shape[0], channels, grid[0], grid[1]).contiguous()

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
                 control_glyph: Optional[torch.FloatTensor] = None, image: PipelineImageInput = None,
                 mask_image: PipelineImageInput = None, strength: float = 0.6):
        """The base call's arguments, ``latents`` being the NOISE here, plus ``image`` (the source: an image, or packed latents
        [B, N, 64]), ``mask_image`` (1 = repaint: an image, or a packed mask [1 or B, N, 64] whose fractional values blend; None: the
        union of the ``control_mask`` images) and ``strength`` (the share of the schedule that runs)."""
        start = RepaintArguments(image, mask_image, strength, control_mask)
        if prompt is not None or prompt_embeds is not None:              # else check_inputs refuses the call
            self._check_repaint_inputs(start, self._batch_size(prompt, prompt_embeds) * num_images_per_prompt,
                                       height or self.default_sample_size * self.vae_scale_factor,
                                       width or self.default_sample_size * self.vae_scale_factor,
                                       len(timesteps) if timesteps is not None else num_inference_steps)
        return self._generate(start, prompt, prompt_2, height, width, num_inference_steps, timesteps, guidance_scale, control_guidance_start,
                              control_guidance_end, control_image, control_mode, controlnet_conditioning_scale, controlnet_conditioning_step,
                              num_images_per_prompt, generator, latents, prompt_embeds, pooled_prompt_embeds, output_type, return_dict,
                              joint_attention_kwargs, callback_on_step_end, callback_on_step_end_tensor_inputs, max_sequence_length,
                              control_mask, control_position, control_glyph)
