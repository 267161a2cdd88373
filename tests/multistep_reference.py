"""Reference of the second-order multistep solver (reptext_amd.scheduler.FlowMatchMultistepScheduler). Not a test module:
test_multistep_host.py, test_multistep_step_kernel_gpu.py and test_multistep_gpu.py import it.

The rule is Adams–Bashforth 2 on the sigma grid of the Euler scheduler:

    x_{i+1} = x_i + dσ_i·(v_i + w_i·(v_i − v_{i−1})),    dσ_i = σ_{i+1} − σ_i,    w_i = dσ_i / (2·dσ_{i−1})

and w = 0 for the first step of a run (no velocity before it: an Euler step). On a uniform grid w = 1/2 and the bracket is the textbook
3/2·v_i − 1/2·v_{i−1}. Three things are here:

``weights``                an fp64 restatement of ``scheduler.multistep_weights`` (written from the formula, not from that function);
``integrate``              the rule over any velocity callable, in the dtype of the state it is given (the host test runs it in fp64);
``denoise_loop_multistep`` the denoising loop, assembled from the oracle's model forwards like tests/cfg_reference.py and
                           tests/repaint_reference.py, whose step bodies it follows line for line: the towers of a step summed as
                           tests/union_reference.py does, under true CFG the conditioning batch cat([negative, positive]) and the mix
                           in fp32, under a repaint the start state, the run from ``t_start`` and the blend after the step.

Rounding under ``orc.stored_as`` happens where the HIP loop rounds: the model outputs (the velocity's halves) and the tower sums. The
state, the mixed velocity and the history stay fp32: the history holds the fp32 velocity the step formed, it is never stored in bf16."""
from typing import Callable, List, Optional, Sequence

import torch

from oracle import flux_oracle as orc


def weights(sigmas, begin: int = 0, order: int = 2) -> List[float]:
    """w_i for i < n = len(sigmas) − 1; 0 up to and including ``begin`` and everywhere at order 1."""
    s = [float(x) for x in sigmas]
    out = []
    for i in range(len(s) - 1):
        first_order = order == 1 or i <= begin
        out.append(0.0 if first_order else (s[i + 1] - s[i]) / (2.0 * (s[i] - s[i - 1])))
    return out


def integrate(velocity: Callable, x, sigmas, begin: int = 0, order: int = 2, restart_at: Sequence[int] = ()):
    """x after the steps begin..n−1 of the rule with ``velocity(x, sigma)``; a step listed in ``restart_at`` forgets the velocity
    before it (first order), as the first step does."""
    s = [float(v) for v in sigmas]
    w = weights(s, begin, order)
    prev = None
    for i in range(begin, len(s) - 1):
        v = velocity(x, s[i])
        if i in restart_at:
            prev = None
        v2 = v if prev is None or w[i] == 0.0 else v + w[i] * (v - prev)
        x = x + (s[i + 1] - s[i]) * v2
        prev = v
    return x


def denoise_loop_multistep(tp, tcfg: dict, cp, ccfg: Optional[dict], latents, prompt_embeds, pooled, control_images: Sequence[torch.Tensor],
                           control_masks: Sequence[Optional[torch.Tensor]], sigmas, img_ids, txt_ids, guidance_scale: float,
                           conditioning_scale: float = 1.0, conditioning_step: int = 10 ** 9, negative: Optional[dict] = None,
                           repaint: Optional[dict] = None, order: int = 2, restart_at: Sequence[int] = ()):
    """The arguments of ``orc.denoise_loop``; ``negative``: dict(prompt_embeds, pooled, scale), the record of
    tests/repaint_reference.py; ``repaint``: dict(src, noise, mask, t_start) — ``latents`` is then ignored, the run starts from the
    source re-noised to sigma[t_start] and its first step is first order. ``order`` 1 is the Euler loop. ``restart_at``: steps (counted
    over the steps that run) that forget the velocity before them, as after a callback that replaced the latents."""
    B = (repaint["src"] if repaint is not None else latents).shape[0]
    rep = (lambda t: torch.cat([t, t], dim=0)) if negative is not None else (lambda t: t)
    pe = torch.cat([negative["prompt_embeds"], prompt_embeds], dim=0) if negative is not None else prompt_embeds
    pl = torch.cat([negative["pooled"], pooled], dim=0) if negative is not None else pooled
    hints = [rep(c) for c in control_images]
    masks = [m if m is None or m.shape[0] == 1 else rep(m) for m in control_masks]
    t_start = repaint["t_start"] if repaint is not None else 0
    w = weights(sigmas, t_start, order)[t_start:]
    sig = sigmas[t_start:]
    n = len(sig) - 1
    if repaint is not None:
        src, noise, mask = repaint["src"].float(), repaint["noise"].float(), repaint["mask"]
        s0 = float(sig[0])
        latents = (1.0 - s0) * src + s0 * noise
    latents = latents.float()
    hist = None
    n_samples = ccfg["num_layers"] if ccfg is not None else 0
    for i in range(n):
        lat_in = rep(latents)
        Bc = lat_in.shape[0]
        timestep = orc._model_t(sig[i] * 1000.0).expand(Bc)
        guidance = torch.full((Bc,), float(guidance_scale)) if tcfg.get("guidance_embeds", False) else None
        merged = [None] * n_samples
        if i < conditioning_step and cp is not None:
            for line, cond in enumerate(hints):
                samples, _ = orc.controlnet_forward(cp, ccfg, lat_in, cond, pe, pl, timestep, img_ids, txt_ids, guidance=guidance,
                                                    conditioning_scale=conditioning_scale, _store_samples=False)
                m = masks[line] if len(masks) > 0 else None
                if m is not None:
                    samples = [m * s for s in samples]
                for j, s in enumerate(samples):
                    merged[j] = orc._s(s) if merged[j] is None else orc._s(merged[j] + s)
        block_samples = None if all(m is None for m in merged) else merged
        v = orc.transformer_forward(tp, tcfg, lat_in, pe, pl, timestep, img_ids, txt_ids, guidance=guidance, controlnet_block_samples=block_samples)
        vel = (v if negative is None else v[:B] + float(negative["scale"]) * (v[B:] - v[:B])).float()      # fp32, not rounded under stored_as
        if i in restart_at:
            hist = None
        vel2 = vel if hist is None or w[i] == 0.0 else vel + w[i] * (vel - hist)
        hist = vel
        sn = float(sig[i + 1])
        r = latents + (sn - float(sig[i])) * vel2
        if repaint is not None:
            kept = (1.0 - sn) * src + sn * noise
            latents = (1.0 - mask) * kept + mask * r
        else:
            latents = r
    return latents
