"""Reference of the repaint loop (latent-blend inpainting), assembled from the oracle's model forwards. Not a test module:
test_repaint_gpu.py imports it.

The contract of pipeline._denoise_eager with ``extras.repaint`` (a pipeline.Repaint): the loop walks ``sigmas[t_start:]`` of the full
text-to-image schedule from the start state (1 − σ_start)·src + σ_start·noise, and every step ends with the blend

    r    = x + (σ_{i+1} − σ_i)·vel            vel: the velocity, or v_neg + s·(v_pos − v_neg) under true CFG
    keep = (1 − σ_{i+1})·src + σ_{i+1}·noise
    x    = (1 − m)·keep + m·r

in fp32 and NOT rounded under ``orc.stored_as`` (the state is the fp32 master copy; rt_repaint_euler_step_f32 forms all of it in one
kernel), while the velocity's halves are rounded to the storage dtype like any model output. Steps are counted over the steps that
run: the text towers are on while ``i < conditioning_step`` and the union tower inside its interval of THOSE steps. The towers of a step
are summed as tests/union_reference.py does (union first, then the text lines; rounded per added tower); under true CFG the
conditioning batch is cat([negative, positive]) against latents, source, noise and mask of batch B, as tests/cfg_reference.py has it.
``blend=False`` leaves the blend out (the plain loop from the same start): the distance between the two is what the test's condition
on its inputs measures."""
from typing import Optional, Sequence

import torch

from oracle import flux_oracle as orc
from union_reference import active_steps


def denoise_loop_repaint(tp, tcfg: dict, cp, ccfg: dict, src, noise, mask, prompt_embeds, pooled, control_images: Sequence[torch.Tensor],
                         control_masks: Sequence[Optional[torch.Tensor]], sigmas, t_start: int, img_ids, txt_ids, guidance_scale: float,
                         conditioning_scale: float = 1.0, conditioning_step: int = 10 ** 9, union: Optional[dict] = None,
                         negative: Optional[dict] = None, blend: bool = True):
    """src, noise [B,N,64] fp32; mask [1 or B,N,64]; sigmas: the FULL schedule with its trailing 0. union: dict(params, cfg, cond
    [B,N,64], scale, start, end). negative: dict(prompt_embeds, pooled, scale)."""
    B = src.shape[0]
    rep = (lambda t: torch.cat([t, t], dim=0)) if negative is not None else (lambda t: t)
    pe = torch.cat([negative["prompt_embeds"], prompt_embeds], dim=0) if negative is not None else prompt_embeds
    pl = torch.cat([negative["pooled"], pooled], dim=0) if negative is not None else pooled
    hints = [rep(c) for c in control_images]
    masks = [m if m is None or m.shape[0] == 1 else rep(m) for m in control_masks]
    ucond = rep(union["cond"]) if union is not None else None
    sig = sigmas[t_start:]
    n = len(sig) - 1
    keep_union = set(active_steps(n, union["start"], union["end"])) if union is not None else set()
    n_samples = ccfg["num_layers"]
    s0 = float(sig[0])
    latents = (1.0 - s0) * src.float() + s0 * noise.float()
    for i in range(n):
        lat_in = rep(latents)
        Bc = lat_in.shape[0]
        timestep = orc._model_t(sig[i] * 1000.0).expand(Bc)
        guidance = torch.full((Bc,), float(guidance_scale)) if tcfg.get("guidance_embeds", False) else None
        merged = [None] * n_samples

        def add(samples):
            for j, s in enumerate(samples):
                merged[j] = orc._s(s) if merged[j] is None else orc._s(merged[j] + s)

        if i in keep_union:
            us, _ = orc.controlnet_forward(union["params"], union["cfg"], lat_in, ucond, pe, pl, timestep, img_ids, txt_ids, guidance=guidance,
                                           conditioning_scale=union["scale"], _store_samples=False)
            add(us)
        if i < conditioning_step:
            for line, cond in enumerate(hints):
                samples, _ = orc.controlnet_forward(cp, ccfg, lat_in, cond, pe, pl, timestep, img_ids, txt_ids, guidance=guidance,
                                                    conditioning_scale=conditioning_scale, _store_samples=False)
                m = masks[line] if len(masks) > 0 else None
                if m is not None:
                    samples = [m * s for s in samples]
                add(samples)
        if all(m is None for m in merged):
            block_samples = None
        else:
            zero = next(m for m in merged if m is not None) * 0.0
            block_samples = [zero if m is None else m for m in merged]
        v = orc.transformer_forward(tp, tcfg, lat_in, pe, pl, timestep, img_ids, txt_ids, guidance=guidance, controlnet_block_samples=block_samples)
        vel = v if negative is None else v[:B] + float(negative["scale"]) * (v[B:] - v[:B])            # fp32, not rounded under stored_as
        sn = float(sig[i + 1])
        r = latents.float() + (sn - float(sig[i])) * vel.float()
        if blend:
            kept = (1.0 - sn) * src.float() + sn * noise.float()
            latents = (1.0 - mask) * kept + mask * r
        else:
            latents = r
    return latents
