"""FluxControlNetPipeline, inpainting variant (RepText tower + a second, inpaint ControlNet + true CFG).

Interface parity target: /root/reference/RepText/pipeline_flux_controlnet_inpaint.py (same class name, other module)
  * constructor with ``controlnet_inpaint`` and a binarising mask processor ........ INP:195-239
  * encode_prompt with negative prompt ............................................. INP:333-448
  * prepare_latents_reptext where the glyph blend IS the initial noise ............. INP:598-653 (vs quirk Q1 of the base)
  * prepare_image_with_mask (masked image -> latents ‖ nearest-resized 1-mask) .... INP:761-826
  * __call__ keywords ............................................................... INP:846-883
  * loop: text towers (masked, summed) + inpaint tower (unmasked) + CFG mix with a zero first step (Q6,Q7,Q8) ... INP:1138-1285
This file holds only what the inpaint flow adds: the negative prompt, the masked-image hint, and a ``__call__`` that hands the
inpaint tower and the CFG mix to the base class's loop (``_denoise_eager``: ``LoopExtras.extra_towers``, ``.velocity``). The stages of
the call (hints, schedule, initial latents, decode) and the loop itself live in pipeline.py, once.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Union

import torch
import torch.nn.functional as F

from . import ops
from .image_processor import PipelineImageInput, VaeImageProcessor
from .pipeline import FluxControlNetPipeline as _BasePipeline
from .pipeline import (ISOLATION_ARGUMENTS, LINE_PROMPT_ARGUMENTS, LINE_SCALE_ARGUMENTS, PAG_ARGUMENTS, REGIONAL_IP_ARGUMENTS, LoopExtras,
                       accepts_call_extensions)

DEFAULT_NEGATIVE_PROMPT = "bad quality, worst quality, text, signature, watermark, extra words"     # INP:416


class FluxControlNetPipeline(_BasePipeline):
    def __init__(self, scheduler, vae, text_encoder, tokenizer, text_encoder_2, tokenizer_2, transformer, controlnet,
                 controlnet_inpaint):
        super().__init__(scheduler, vae, text_encoder, tokenizer, text_encoder_2, tokenizer_2, transformer, controlnet)
        self.controlnet_inpaint = controlnet_inpaint
        self.mask_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_resize=True, do_convert_grayscale=True,
                                                do_normalize=False, do_binarize=True)

    @property
    def components(self) -> Dict[str, Any]:
        c = super().components
        c["controlnet_inpaint"] = self.controlnet_inpaint
        return c

    # ------------------------------------------------------------------ INP:333-448
    def encode_prompt(self, prompt, prompt_2, device=None, num_images_per_prompt: int = 1, do_classifier_free_guidance: bool = True,
                      negative_prompt=None, negative_prompt_2=None, prompt_embeds=None, pooled_prompt_embeds=None,
                      max_sequence_length: int = 512, lora_scale=None, negative_prompt_embeds=None,
                      negative_pooled_prompt_embeds=None):
        """Returns (prompt_embeds, pooled, negative_prompt_embeds, negative_pooled, text_ids). Pre-computed negative
        embeddings may be passed (extension) when the pipeline has no text encoders."""
        pe, pooled, text_ids = super().encode_prompt(prompt, prompt_2, device=device, num_images_per_prompt=num_images_per_prompt,
                                                     prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                                                     max_sequence_length=max_sequence_length)
        npe = npooled = None
        if do_classifier_free_guidance:
            if negative_prompt_embeds is not None:
                npe, npooled = negative_prompt_embeds, negative_pooled_prompt_embeds
            else:
                batch = pe.shape[0] // num_images_per_prompt            # one negative string serves every prompt of the batch
                per_prompt = lambda p: [p] * batch if isinstance(p, str) else p
                neg = per_prompt(negative_prompt or DEFAULT_NEGATIVE_PROMPT)
                neg2 = per_prompt(negative_prompt_2) if negative_prompt_2 else neg
                npooled = self._get_clip_prompt_embeds(neg, num_images_per_prompt, device)
                npe = self._get_t5_prompt_embeds(neg2, num_images_per_prompt, max_sequence_length, device)
        return pe, pooled, npe, npooled, text_ids

    glyph_blend_is_initial_latents = True      # INP:645-647: prepare_latents_reptext returns the glyph blend (the base drops it, Q1)

    # ------------------------------------------------------------------ INP:761-826
    def prepare_image_with_mask(self, image, mask, width, height, batch_size, num_images_per_prompt, device, dtype,
                                do_classifier_free_guidance=False):
        """Masked source image (masked pixels = -1) -> VAE latents (global-RNG posterior sample, Q2), concatenated with the
        nearest-resized inverted mask as a 17th channel, packed -> [B, N, 68]."""
        image = self._prep_pixels(image, width, height, batch_size, num_images_per_prompt, device, dtype)
        mask = self._prep_pixels(mask, width, height, batch_size, num_images_per_prompt, device, dtype, processor=self.mask_processor)
        masked = torch.where((mask > 0.5).repeat(1, 3, 1, 1), torch.full_like(image, -1.0), image)
        lat = self.vae.encode(masked.to(self.vae.dtype)).latent_dist.sample()
        lat = ((lat - self.vae.config.shift_factor) * self.vae.config.scaling_factor).to(dtype)
        msize = (height // self.vae_scale_factor * 2, width // self.vae_scale_factor * 2)
        m = (ops.resize2d(mask.float(), size=msize, mode="nearest") if mask.is_cuda else F.interpolate(mask.float(), size=msize)).to(dtype)
        both = torch.cat([lat, 1 - m], dim=1)
        packed = self._pack_latents(both, batch_size * num_images_per_prompt, both.shape[1], both.shape[2], both.shape[3])
        if do_classifier_free_guidance:
            packed = torch.cat([packed] * 2)
        return packed, height, width

    # ------------------------------------------------------------------ INP:846-1313
    @accepts_call_extensions("ip_adapter_image", "ip_adapter_image_embeds", *LINE_PROMPT_ARGUMENTS, *REGIONAL_IP_ARGUMENTS,
                             *ISOLATION_ARGUMENTS, *LINE_SCALE_ARGUMENTS, *PAG_ARGUMENTS)      # taken only to be refused by name below
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]] = None, prompt_2: Optional[Union[str, List[str]]] = None,
                 true_guidance_scale: float = 3.5, negative_prompt: Optional[Union[str, List[str]]] = None,
                 negative_prompt_2: Optional[Union[str, List[str]]] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 28, timesteps: List[int] = None, guidance_scale: float = 7.0,
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
                 control_glyph: Optional[torch.FloatTensor] = None, control_image_inpaint: PipelineImageInput = None,
                 control_mask_inpaint: Optional[torch.FloatTensor] = None,
                 controlnet_conditioning_scale_inpaint: Union[float, List[float]] = 1.0,
                 negative_prompt_embeds: Optional[torch.FloatTensor] = None,
                 negative_pooled_prompt_embeds: Optional[torch.FloatTensor] = None):
        if self.guider is not None:
            # this flow keeps the reference's own CFG (LoopExtras.velocity, the zero-velocity first step): no interval, no projection
            raise ValueError("the inpaint pipeline does not support pipe.guider (a guidance interval or projected guidance); set it to None")
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        self.check_inputs(prompt, prompt_2, height, width, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                          callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, max_sequence_length=max_sequence_length)
        ext = self._call_extensions
        if ext.ip_adapter_image is not None or ext.ip_adapter_image_embeds is not None or "ip_adapter_image_embeds" in (joint_attention_kwargs or {}):
            # the conditioning batch is 2B under true CFG: the unconditional half would need a negative image prompt
            raise ValueError("the inpaint pipeline does not support IP-Adapter image prompts (ip_adapter_image / ip_adapter_image_embeds)")
        if any(getattr(ext, k, None) is not None for k in REGIONAL_IP_ARGUMENTS[:3]):
            raise ValueError("the inpaint pipeline does not support IP-Adapter image prompts (ip_adapter_mask / control_ip_adapter_image / "
                             "control_ip_adapter_image_embeds)")
        if getattr(ext, "control_prompt", None) is not None or getattr(ext, "control_prompt_embeds", None) is not None:
            # the flow's own CFG doubles the batch inside the loop: the row table of the unconditional half is not built for it
            raise ValueError("the inpaint pipeline does not support per-line prompts (control_prompt / control_prompt_embeds)")
        if getattr(ext, "control_prompt_isolation", False):
            raise ValueError("the inpaint pipeline does not support per-line prompts (control_prompt_isolation)")
        if getattr(ext, "control_prompt_scale", None) is not None:
            raise ValueError("the inpaint pipeline does not support per-line prompts (control_prompt_scale)")
        if getattr(ext, "pag_scale", 0.0) or getattr(ext, "pag_applied_layers", None) is not None:
            raise ValueError("the inpaint pipeline does not support perturbed-attention guidance (pag_scale / pag_applied_layers)")
        if getattr(self.scheduler, "stochastic_sampling", False):
            raise ValueError("the inpaint pipeline does not support stochastic sampling (the scheduler's stochastic_sampling)")
        self._guidance_scale, self._joint_attention_kwargs, self._interrupt = guidance_scale, joint_attention_kwargs, False
        cfg = self.do_classifier_free_guidance                          # enabled by guidance_scale > 1, scaled by true_guidance_scale (Q8)
        device, dtype = self._execution_device, self.transformer.dtype
        total = self._batch_size(prompt, prompt_embeds) * num_images_per_prompt
        # INP:1033-1035,1145: latents keep batch B while the conditioning is 2B = cat([negative × B, positive × B]). The reference only
        # broadcasts for B == 1 (Q6); a larger batch is this project's: the models repeat the latents over the conditioning batch, hints
        # and per-image masks are doubled, and chunk(2) below splits the velocity into its negative and positive halves.

        pe, pooled, npe, npooled, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            do_classifier_free_guidance=cfg, negative_prompt=negative_prompt, negative_prompt_2=negative_prompt_2, device=device,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length,
            negative_prompt_embeds=negative_prompt_embeds, negative_pooled_prompt_embeds=negative_pooled_prompt_embeds)
        pe, pooled = pe.to(device), pooled.to(device)
        if cfg:
            pe = torch.cat([npe.to(device), pe], dim=0)                 # negative first (INP:1034-1035)
            pooled = torch.cat([npooled.to(device), pooled], dim=0)

        hints, height, width = self._collect_hints(control_image, control_position, height, width, total, num_images_per_prompt, device,
                                                   dtype, cfg=cfg)
        if self._is_packed_hint(control_image_inpaint, self.controlnet_inpaint):
            hint_inp = self._doubled_under_cfg(control_image_inpaint.to(device=device, dtype=dtype), total, cfg)
        else:
            hint_inp, height, width = self.prepare_image_with_mask(image=control_image_inpaint, mask=control_mask_inpaint, width=width,
                                                                   height=height, batch_size=total, num_images_per_prompt=num_images_per_prompt,
                                                                   device=device, dtype=dtype, do_classifier_free_guidance=cfg)
        timesteps, num_inference_steps = self._schedule(height, width, num_inference_steps, timesteps, device)
        latents, image_ids = self._initial_latents(control_glyph, total, height, width, pe.dtype, device, generator, latents)
        masks = [self._doubled_under_cfg(m, total, cfg, mask=True) for m in self._region_masks(control_mask, latents.device, latents.dtype)]

        def cfg_velocity(i, noise_pred):
            """True CFG on the two halves of the conditioning batch (negative first, INP:1264-1270); zero velocity at step 0 (Q7)."""
            uncond, text = noise_pred.chunk(2)
            return ops.cfg_mix(uncond, text, float(true_guidance_scale)) if i > 0 else torch.zeros_like(text)

        self._apply_lora_scale()
        # The shared loop, always eager here (no graph capture, no tower side stream): the inpaint tower follows the text-line towers
        tvals = timesteps.to(torch.float32).cpu().tolist()
        latents = self._denoise_eager(latents, pe, pooled, text_ids, image_ids, tvals, hints, masks, guidance_scale,
                                      controlnet_conditioning_scale, controlnet_conditioning_step, control_mode, callback_on_step_end,
                                      callback_on_step_end_tensor_inputs, num_inference_steps, timesteps,
                                      extras=LoopExtras(extra_towers=((self.controlnet_inpaint, hint_inp, controlnet_conditioning_scale_inpaint),),
                                                        velocity=cfg_velocity if cfg else None))
        return self._finish(latents, height, width, output_type, return_dict)
