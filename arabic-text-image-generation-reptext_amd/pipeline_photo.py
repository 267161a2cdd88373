"""FluxControlNetPhotoPipeline: the repaint call on a photo of any size.

The repaint pipeline renders text into an image that already has the working size and returns pixels that all went through the VAE.
This one takes the photo as it is: it cuts the region around the mask out of it, resamples that region — and every conditioning image
with it — to the working size, runs the repaint call unchanged, resamples the decoded image back and blends it into the untouched
photo under a feathered mask. The pixels away from the mask are the photo's bytes, at the photo's resolution, and the model's working
size is spent on the region, not on the whole picture. All pixel work is on the device (csrc/photo.hip: rt_resize_aa,
rt_gaussian_blur_f32, rt_composite_u8); the photo crosses the bus once in each direction, as uint8.

The rules (``padding_mask_crop``, the crop region grown to the working aspect, the blurred-mask overlay) are diffusers'
``get_crop_region`` / ``apply_overlay`` and A1111's mask blur as recalled — neither is installed: rules recalled, parity unpinned
(DESIGN.md §7). What is pinned: ``photo_crop_region``'s known answers, the kernels per element against fp64, and the bitwise
properties of the call (tests/test_photo_*.py).

This file holds what the flow adds around the repaint call: the region, the refusals (host-side, before any device work), the resampling
of the inputs, and the paste-back. The loop, its graph key and its static inputs are the repaint call's.
"""
from __future__ import annotations

import math
from dataclasses import replace
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from PIL import Image

from . import native, ops
from .image_processor import PipelineImageInput
from .pipeline import PerturbedCallExtensions, FluxPipelineOutput, accepts_call_extensions
from .pipeline_repaint import FluxControlNetRepaintPipeline, RepaintArguments

MASK_THRESHOLD = 128            # a uint8 mask value counts as "repaint" from here on: x/255 >= 0.5


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def _grown_to_aspect(w: int, h: int, work_w: int, work_h: int) -> Tuple[int, int]:
    """The smallest (w', h') >= (w, h) with w' : h' = work_w : work_h up to the ceil of the side that grows."""
    if w * work_h < h * work_w:
        return _ceil_div(h * work_w, work_h), h
    return w, _ceil_div(w * work_h, work_w)


def _fitting_work_size(w: int, h: int, photo_w: int, photo_h: int, work_w: int, work_h: int) -> Optional[Tuple[int, int]]:
    """A working size (multiples of 16, no larger than the one asked for) whose aspect the ``w`` x ``h`` box can be grown to inside the
    photo: the asked size with one side shortened to the box's reach, else the photo's own aspect. None when neither fits."""
    long_side = max(work_w, work_h)
    candidates = [(min(work_w, max(16, photo_w * work_h // h // 16 * 16)), work_h), (work_w, min(work_h, max(16, photo_h * work_w // w // 16 * 16)))]
    scale = long_side / max(photo_w, photo_h)
    candidates.append((max(16, int(photo_w * scale) // 16 * 16), max(16, int(photo_h * scale) // 16 * 16)))
    for cw, ch in candidates:
        gw, gh = _grown_to_aspect(w, h, cw, ch)
        if gw <= photo_w and gh <= photo_h:
            return cw, ch
    return None


def photo_crop_region(bbox, photo_w: int, photo_h: int, pad: int, work_w: int, work_h: int) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1), ends exclusive: the part of a ``photo_w`` x ``photo_h`` photo that is resampled to ``work_w`` x ``work_h``.

    ``bbox`` (x0, y0, x1, y1; ends exclusive) is the bounding box of the mask's pixels. It is grown by ``pad`` on every side and clamped
    to the photo; then the side that is too short for the aspect ``work_w : work_h`` grows about the box's centre to
    ``ceil(other · aspect)`` — of the added pixels ``floor(half)`` go to the left / top, the rest to the right / bottom — and the box is
    shifted back inside the photo. Where the photo is too small in that direction a ``ValueError`` names a working size that fits."""
    bx0, by0, bx1, by1 = (int(v) for v in bbox)
    photo_w, photo_h, pad, work_w, work_h = int(photo_w), int(photo_h), int(pad), int(work_w), int(work_h)
    if not (0 <= bx0 < bx1 <= photo_w and 0 <= by0 < by1 <= photo_h):
        raise ValueError(f"bbox {tuple(bbox)} is empty or not inside the {photo_w}x{photo_h} photo")
    if pad < 0 or work_w < 1 or work_h < 1:
        raise ValueError(f"pad {pad} / working size {work_w}x{work_h}")
    x0, y0, x1, y1 = max(bx0 - pad, 0), max(by0 - pad, 0), min(bx1 + pad, photo_w), min(by1 + pad, photo_h)
    w, h = x1 - x0, y1 - y0
    gw, gh = _grown_to_aspect(w, h, work_w, work_h)
    if gw > photo_w or gh > photo_h:
        fit = _fitting_work_size(w, h, photo_w, photo_h, work_w, work_h)
        hint = f"a working size that fits: width={fit[0]}, height={fit[1]}" if fit else "no working size of this aspect family fits"
        raise ValueError(f"the {photo_w}x{photo_h} photo is too small for a region of aspect {work_w}:{work_h} around the {w}x{h} padded mask box "
                         f"(it would be {gw}x{gh}); {hint}")
    x0 = min(max(x0 - (gw - w) // 2, 0), photo_w - gw)
    y0 = min(max(y0 - (gh - h) // 2, 0), photo_h - gh)
    return x0, y0, x0 + gw, y0 + gh


def min_padding_for_blur(mask_blur: float) -> int:
    """The smallest ``padding_mask_crop`` under which the feather (radius ceil(3·sigma)) stays inside the region."""
    return int(math.ceil(3.0 * float(mask_blur)))


def _single(x, name: str):
    """``x`` itself, or the one element of a one-element list."""
    if isinstance(x, (list, tuple)):
        if len(x) != 1:
            raise ValueError(f"`{name}`: one photo per call ({len(x)} given); `num_images_per_prompt` gives several results for it")
        return x[0]
    return x


def _host_u8(x, name: str, gray: bool):
    """uint8 numpy [H,W] (``gray``) or [H,W,3] of a PIL image, a uint8 array or a uint8 tensor."""
    if isinstance(x, Image.Image):
        return np.array(x.convert("L" if gray else "RGB"))            # a copy: writable, so that torch takes it
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if not isinstance(x, np.ndarray) or x.dtype != np.uint8:
        raise ValueError(f"`{name}`: a PIL image, or a uint8 array / tensor at the photo's size (got {type(x).__name__}"
                         f"{' of ' + str(x.dtype) if isinstance(x, np.ndarray) else ''})")
    if x.ndim == 3 and x.shape[-1] == 1:
        x = x[..., 0]
    if gray and x.ndim == 3 and x.shape[-1] == 3:
        x = np.array(Image.fromarray(x).convert("L"))
    if not gray and x.ndim == 2:
        x = np.repeat(x[..., None], 3, axis=2)
    if x.ndim != (2 if gray else 3) or (not gray and x.shape[-1] != 3):
        raise ValueError(f"`{name}`: expected {'[H,W]' if gray else '[H,W,3]'}, got {tuple(x.shape)}")
    return np.ascontiguousarray(x)


class FluxControlNetPhotoPipeline(FluxControlNetRepaintPipeline):
    def _is_token_tensor(self, t) -> bool:
        """A tensor that is no image: packed latents / hints [B, N, C] or a token mask [B, N, 1]. Such a tensor has the working size by
        construction and is handed on as it is."""
        return isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype != torch.uint8

    def _check_photo_inputs(self, image, mask_image, control_image, control_mask, control_position, control_glyph, control_image_union,
                            padding_mask_crop, mask_blur, output_type, height, width):
        """Every refusal of the photo flow, on the host, before any device work. Returns what the call then uploads:
        (photo uint8 [H,W,3] — numpy, or the caller's device tensor —, mask uint8 [H,W], region (x0, y0, x1, y1), and the conditioning images as
        uint8 arrays in the shape of the arguments, token tensors left as they are)."""
        if output_type not in ("pil", "np", "pt", "latent"):
            raise ValueError(f"unsupported output_type {output_type}")
        if image is None:
            raise ValueError("`image` (the photo to repaint) is required")
        image = _single(image, "image")
        if self._is_packed(image) or self._is_packed(mask_image):
            raise ValueError("packed latents as `image` / `mask_image` have the working size already: they belong to FluxControlNetRepaintPipeline")
        if isinstance(image, (torch.Tensor, np.ndarray)) and image.ndim == 4:
            if image.shape[0] != 1:
                raise ValueError(f"`image`: one photo per call ({image.shape[0]} given); `num_images_per_prompt` gives several results for it")
            image = image[0]
        if isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[-1] == 3:
            photo = image.contiguous()                                   # already on the device
        else:
            photo = _host_u8(image, "image", gray=False)
        H, W = int(photo.shape[0]), int(photo.shape[1])
        blur, pad = float(mask_blur), int(padding_mask_crop)
        if not 0.0 <= blur <= native.RT_BLUR_MAX_RADIUS / 3.0:
            raise ValueError(f"`mask_blur` {mask_blur} is outside [0, {native.RT_BLUR_MAX_RADIUS // 3}]")
        if pad < min_padding_for_blur(blur):
            raise ValueError(f"`padding_mask_crop` {pad} is smaller than the feather's radius: with mask_blur={blur} the blurred mask would reach the "
                             f"region's border and leave a seam; the smallest padding_mask_crop that works is {min_padding_for_blur(blur)}")

        def sized(x, name, gray):
            if x is None or self._is_token_tensor(x):
                return x
            a = _host_u8(x, name, gray)
            if a.shape[:2] != (H, W):
                raise ValueError(f"`{name}`: {a.shape[1]}x{a.shape[0]} pixels, but every conditioning image is given at the photo's size {W}x{H}")
            return a

        def sized_list(xs, name, gray):
            if xs is None:
                return None
            if not isinstance(xs, (list, tuple)):
                raise ValueError(f"`{name}`: a list with one image per text line")
            return [sized(x, f"{name}[{i}]", gray) for i, x in enumerate(xs)]

        if mask_image is not None:
            mask, name = _host_u8(_single(mask_image, "mask_image"), "mask_image", True), "mask_image"
        else:
            mask, name = _host_u8(self._union_of_masks(control_mask), "control_mask", True), "control_mask"      # refuses tensors and mixed sizes
        if mask.shape != (H, W):
            raise ValueError(f"`{name}`: {mask.shape[1]}x{mask.shape[0]} pixels, but the mask is given at the photo's size {W}x{H}")
        cond = dict(control_image=sized_list(control_image, "control_image", False), control_mask=sized_list(control_mask, "control_mask", True),
                    control_position=sized_list(control_position, "control_position", True),
                    control_glyph=sized(control_glyph, "control_glyph", False),
                    control_image_union=sized(control_image_union, "control_image_union", False))
        ys, xs = np.nonzero(mask >= MASK_THRESHOLD)
        if ys.size == 0:
            raise ValueError("the mask is empty (no pixel >= 128): there is nothing to repaint")
        bbox = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)
        region = photo_crop_region(bbox, W, H, pad, width, height)
        cw, ch = region[2] - region[0], region[3] - region[1]
        limit = native.RT_RESIZE_AA_MAX_SCALE
        if cw > limit * width or ch > limit * height or width > limit * cw or height > limit * ch:
            raise ValueError(f"the region {cw}x{ch} and the working size {width}x{height} differ by more than a factor of {limit}")
        return photo, mask, region, cond

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
                 mask_image: PipelineImageInput = None, strength: float = 0.6, padding_mask_crop: int = 32, mask_blur: float = 4.0):
        """The repaint call's arguments with ``image`` the PHOTO at any size (PIL, or a uint8 array / tensor [H, W, 3]; one per call) and
        ``mask_image``, ``control_image``, ``control_mask``, ``control_position``, ``control_glyph`` and ``control_image_union`` at the
        photo's size; ``height`` / ``width`` are the working size. ``padding_mask_crop`` pixels are kept around the mask's box when the
        region is cut, ``mask_blur`` is the sigma of the feather under which the result is blended into the photo (0: the binary mask).
        The images returned have the photo's size; ``output_type="latent"`` returns the working-size latents, with no composite.
        A region that already has the working size is not resampled — the way to keep Canny hints pixel-sharp."""
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        ext = self._call_extensions
        if prompt is None and prompt_embeds is None:                     # check_inputs refuses the call
            self.check_inputs(prompt, prompt_2, height, width, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                              callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, max_sequence_length=max_sequence_length)
        photo, mask, region, cond = self._check_photo_inputs(image, mask_image, control_image, control_mask, control_position, control_glyph,
                                                             ext.control_image_union, padding_mask_crop, mask_blur, output_type, height, width)
        self._check_repaint_inputs(RepaintArguments(photo, mask, strength, None), self._batch_size(prompt, prompt_embeds) * num_images_per_prompt,
                                   height, width, len(timesteps) if timesteps is not None else num_inference_steps)

        # ---- crop and resample, on the device
        device = self._execution_device
        window = (region[0], region[1], region[2] - region[0], region[3] - region[1])
        size = (int(height), int(width))
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).to(device)
        photo_d, mask_d = up(photo), up(mask)

        def pixels(a, mul=1.0, add=0.0):
            """uint8 image at the photo's size -> fp32 [1, C, height, width] of the region; None and token tensors pass."""
            if a is None or (isinstance(a, torch.Tensor) and a.dtype != torch.uint8):
                return a
            return ops.resize_aa(up(a), window, size, mul, add)[None]

        def binary(a):
            """a mask or position image -> the region's {0, 1} plane [height, width] (bool), re-binarised at 0.5 after the resample"""
            return ops.resize_aa(up(a), window, size)[0] >= 0.5

        def token_mask(a):
            """what the base call makes of a uint8 mask image at the working size: /255, bilinear x 1/16, [1, N, 1]"""
            if isinstance(a, torch.Tensor):
                return a
            u8 = binary(a).to(torch.uint8) * 255
            return ops.resize2d(u8[None, None], scale_factor=1 / 16, mode="bilinear", u8_scale=255.0).reshape([1, -1, 1])

        work_image = pixels(photo_d)                                                          # [0, 1]: the processor normalises it
        work_mask = binary(mask_d).to(torch.float32)[None, None]
        # hints go to the VAE as they are when they are tensors: [-1, 1] here (mul 2, add -1), a position as 2·b − 1
        work_hints = None if cond["control_image"] is None else [pixels(a, 2.0, -1.0) for a in cond["control_image"]]
        work_positions = None if cond["control_position"] is None else [
            a if isinstance(a, torch.Tensor) else (binary(a).to(torch.float32) * 2.0 - 1.0)[None, None] for a in cond["control_position"]]
        work_masks = None if cond["control_mask"] is None else [token_mask(a) for a in cond["control_mask"]]
        work_glyph = pixels(cond["control_glyph"])                                            # [0, 1]: preprocessed by the processor
        if cond["control_image_union"] is not None:
            self._call_extensions = replace(ext, control_image_union=pixels(cond["control_image_union"], 2.0, -1.0))

        # ---- the repaint call, unchanged
        start = RepaintArguments(work_image, work_mask, strength, work_masks)
        lat32 = self._generate(start, prompt, prompt_2, height, width, num_inference_steps, timesteps, guidance_scale, control_guidance_start,
                               control_guidance_end, work_hints, control_mode, controlnet_conditioning_scale, controlnet_conditioning_step,
                               num_images_per_prompt, generator, latents, prompt_embeds, pooled_prompt_embeds, "latent", False,
                               joint_attention_kwargs, callback_on_step_end, callback_on_step_end_tensor_inputs, max_sequence_length,
                               work_masks, work_positions, work_glyph)[0]
        if output_type == "latent":
            return FluxPipelineOutput(images=lat32) if return_dict else (lat32,)

        # ---- paste back
        h2, w2 = 2 * (int(height) // self.vae_scale_factor), 2 * (int(width) // self.vae_scale_factor)
        decoded = self.vae.decode_packed(lat32.to(torch.bfloat16), h2, w2)                    # fp32 [B, 3, height, width] in [-1, 1]
        alpha = ops.gaussian_blur((mask_d[region[1]:region[3], region[0]:region[2]] >= MASK_THRESHOLD).to(torch.float32).contiguous(), float(mask_blur))
        out = torch.stack([ops.composite_u8(photo_d, ops.resize_aa(d.contiguous(), None, (window[3], window[2])), alpha, window) for d in decoded])
        if output_type == "pt":
            images = out.permute(0, 3, 1, 2).to(torch.float32) / 255.0
        else:
            images = self.image_processor.postprocess_u8(out, output_type)
        return FluxPipelineOutput(images=images) if return_dict else (images,)
