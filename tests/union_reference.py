"""Reference of the denoising loop with a second, unmasked ControlNet (the union tower) beside the text-line towers, assembled from
the oracle's model forwards. Not a test module: test_union_tower_gpu.py imports it.

Order of the sum within a step (the contract of pipeline._denoise_eager with ``extras.union``, a pipeline.UnionTower): the union tower first, when the step is inside its guidance
interval, then the text lines while ``i < conditioning_step``; the first tower evaluated sets the samples, every later one is added
and the sum is rounded to the storage dtype per added tower (``_s(a + b)``), the regional mask applied before the sum — where
``oracle.flux_oracle.denoise_loop`` rounds."""
from typing import Optional, Sequence

import torch

from oracle import flux_oracle as orc


def active_steps(n: int, start: float, end: float):
    """diffusers' ``controlnet_keep`` (recalled): step i of n runs iff not (i / n < start or (i + 1) / n > end)."""
    return [i for i in range(n) if not (i / n < start or (i + 1) / n > end)]


def denoise_loop_union(tp, tcfg: dict, cp, ccfg: dict, up, ucfg: dict, latents, prompt_embeds, pooled,
                       control_images: Sequence[torch.Tensor], control_masks: Sequence[Optional[torch.Tensor]], union_cond, sigmas,
                       img_ids, txt_ids, guidance_scale: float, conditioning_scale: float = 1.0, conditioning_step: int = 10 ** 9,
                       union_scale: float = 1.0, union_start: float = 0.0, union_end: float = 1.0):
    """latents [B,N,64]; control_images: per text line [B,N,128]; control_masks: per line [1,N,1] or None; union_cond [B,N,64].
    The samples keep the FIRST tower's depth (``ccfg``): a shallower union tower adds into the leading ones."""
    B = latents.shape[0]
    n = len(sigmas) - 1
    n_samples = ccfg["num_layers"]
    keep = set(active_steps(n, union_start, union_end))
    for i in range(n):
        timestep = orc._model_t(sigmas[i] * 1000.0).expand(B)
        guidance = torch.full((B,), float(guidance_scale)) if tcfg.get("guidance_embeds", False) else None
        merged = [None] * n_samples

        def add(samples):
            for j, s in enumerate(samples):
                merged[j] = orc._s(s) if merged[j] is None else orc._s(merged[j] + s)

        if i in keep:
            us, _ = orc.controlnet_forward(up, ucfg, latents, union_cond, prompt_embeds, pooled, timestep, img_ids, txt_ids,
                                           guidance=guidance, conditioning_scale=union_scale, _store_samples=False)
            add(us)
        if i < conditioning_step:
            for line, cond in enumerate(control_images):
                samples, _ = orc.controlnet_forward(cp, ccfg, latents, cond, prompt_embeds, pooled, timestep, img_ids, txt_ids,
                                                    guidance=guidance, conditioning_scale=conditioning_scale, _store_samples=False)
                mask = control_masks[line] if len(control_masks) > 0 else None
                if mask is not None:
                    samples = [mask * s for s in samples]
                add(samples)
        if all(m is None for m in merged):
            block_samples = None
        else:
            zero = next(m for m in merged if m is not None) * 0.0
            block_samples = [zero if m is None else m for m in merged]
        v = orc.transformer_forward(tp, tcfg, latents, prompt_embeds, pooled, timestep, img_ids, txt_ids, guidance=guidance,
                                    controlnet_block_samples=block_samples)
        latents = orc.euler_step(latents, v, float(sigmas[i]), float(sigmas[i + 1]))
    return latents
