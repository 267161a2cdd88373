"""Reference of the text-to-image denoising loop under true CFG (a negative prompt), assembled from the oracle's model forwards.
Not a test module: test_true_cfg_gpu.py imports it.

The contract of pipeline._denoise_eager with ``extras.cfg_scale`` (pipeline.LoopExtras): the conditioning batch is
cat([negative, positive]) against latents of batch B, which the models see repeated ([lat_0..lat_{B-1}, lat_0..]); hints, the union hint and per-image masks are doubled the same
way, a shared [1,N,1] mask serves both halves; at EVERY step (no zero-velocity first step: that quirk is the inpaint pipeline's)

    latents <- latents + (sigma_{i+1} - sigma_i) · (v_neg + s · (v_pos - v_neg))

with the two halves of the transformer's output rounded to the storage dtype under ``orc.stored_as`` like any velocity, and the mix
itself NOT rounded: it is formed in fp32 inside the step (rt_cfg_euler_step_f32). The towers of a step are summed as
tests/union_reference.py does (union tower first, inside its interval; then the text lines while ``i < conditioning_step``). The image
prompt, when there is one, is ``cat([negative embeds, positive embeds])`` through the restatement whose ``transformer_forward`` is
passed in (tests/ip_adapter_reference.py for the diffusers / XLabs layouts, tests/instantx_reference.py for InstantX)."""
from typing import Optional, Sequence

import torch

from oracle import flux_oracle as orc
from union_reference import active_steps


def denoise_loop_cfg(tp, tcfg: dict, cp, ccfg: Optional[dict], latents, prompt_embeds, pooled, neg_prompt_embeds, neg_pooled,
                     control_images: Sequence[torch.Tensor], control_masks: Sequence[Optional[torch.Tensor]], sigmas, img_ids, txt_ids,
                     guidance_scale: float, true_cfg_scale: float, conditioning_scale: float = 1.0, conditioning_step: int = 10 ** 9,
                     union: Optional[dict] = None, image_prompt: Optional[dict] = None):
    """latents [B,N,64]; control_images per text line [B,N,128]; control_masks per line [1,N,1], [B,N,1] or None.
    union: dict(params, cfg, cond [B,N,64], scale, start, end). image_prompt: dict(forward, ip_params, ip_scales, embeds [B,E],
    neg_embeds [B,E])."""
    B = latents.shape[0]
    two = lambda t: torch.cat([t, t], dim=0)
    pe = torch.cat([neg_prompt_embeds, prompt_embeds], dim=0)
    pl = torch.cat([neg_pooled, pooled], dim=0)
    hints = [two(c) for c in control_images]
    masks = [m if m is None or m.shape[0] == 1 else two(m) for m in control_masks]
    ucond = two(union["cond"]) if union is not None else None
    forward, fkw = orc.transformer_forward, {}
    if image_prompt is not None:
        forward = image_prompt["forward"]
        fkw = dict(ip_params=image_prompt["ip_params"], ip_scales=image_prompt["ip_scales"],
                   ip_embeds=torch.cat([image_prompt["neg_embeds"], image_prompt["embeds"]], dim=0))
    n = len(sigmas) - 1
    keep = set(active_steps(n, union["start"], union["end"])) if union is not None else set()
    n_samples = ccfg["num_layers"] if ccfg is not None else 0
    for i in range(n):
        lat_in = two(latents)
        timestep = orc._model_t(sigmas[i] * 1000.0).expand(2 * B)
        guidance = torch.full((2 * B,), float(guidance_scale)) if tcfg.get("guidance_embeds", False) else None
        merged = [None] * n_samples

        def add(samples):
            for j, s in enumerate(samples):
                merged[j] = orc._s(s) if merged[j] is None else orc._s(merged[j] + s)

        if i in keep:
            us, _ = orc.controlnet_forward(union["params"], union["cfg"], lat_in, ucond, pe, pl, timestep, img_ids, txt_ids, guidance=guidance,
                                           conditioning_scale=union["scale"], _store_samples=False)
            add(us)
        if i < conditioning_step and cp is not None:
            for line, cond in enumerate(hints):
                samples, _ = orc.controlnet_forward(cp, ccfg, lat_in, cond, pe, pl, timestep, img_ids, txt_ids, guidance=guidance,
                                                    conditioning_scale=conditioning_scale, _store_samples=False)
                mask = masks[line] if len(masks) > 0 else None
                if mask is not None:
                    samples = [mask * s for s in samples]
                add(samples)
        if all(m is None for m in merged):
            block_samples = None
        else:
            zero = next(m for m in merged if m is not None) * 0.0
            block_samples = [zero if m is None else m for m in merged]
        v = forward(tp, tcfg, lat_in, pe, pl, timestep, img_ids, txt_ids, guidance=guidance, controlnet_block_samples=block_samples, **fkw)
        v_neg, v_pos = v[:B], v[B:]
        mixed = v_neg + float(true_cfg_scale) * (v_pos - v_neg)                      # fp32, not rounded under stored_as
        latents = orc.euler_step(latents, mixed, float(sigmas[i]), float(sigmas[i + 1]))
    return latents
