"""The reference of the denoising loop with every extension pipeline._denoise_eager takes as ``LoopExtras`` — the union tower, true
CFG, a repaint, the multistep scheduler, a guider, an image prompt — in any combination, assembled from the oracle's model forwards.
Not a test module: the loop tests (union tower, true CFG, repaint, multistep, guidance) and the step-kernel tests import it.

``active_steps``            diffusers' ``controlnet_keep``: the steps of an interval given as fractions of the run.
``weights``                 an fp64 restatement of ``scheduler.multistep_weights`` (written from the formula, not from that function).
``integrate``               the multistep rule over any velocity callable, in the dtype of the state it is given.
``projected_velocity``      the rule of a guided step, per sample, in float64 (the kernel tests' reference).
``denoise_loop_reference``  the loop. Without extensions it returns ``oracle.flux_oracle.denoise_loop``'s bits.

The multistep rule is Adams–Bashforth 2 on the sigma grid of the Euler scheduler:

    x_{i+1} = x_i + dσ_i·(v_i + w_i·(v_i − v_{i−1})),    dσ_i = σ_{i+1} − σ_i,    w_i = dσ_i / (2·dσ_{i−1})

and w = 0 for the first step of a run (no velocity before it: an Euler step). On a uniform grid w = 1/2 and the bracket is the textbook
3/2·v_i − 1/2·v_{i−1}. The rule of a guided step under a guider that projects (p, u the positive and negative halves of the velocity):

    d = (p − u) + β·r_prev;   a = Σ d², b = Σ d·p, c = Σ p²;   k = τ > 0 and a > τ² ? τ/√a : 1;   α = c > 0 ? k·b/c : 0
    v = p + (s − 1)·(k·d + (η − 1)·α·p)

Rounding under ``orc.stored_as`` happens where the HIP loop rounds: the model outputs (the velocity's halves) and the tower sums. The
state, the mixed or guided velocity, d and the multistep history stay fp32 and are never rounded: the step kernels form them in fp32
from the fp32 master copy."""
from typing import Callable, List, Optional, Sequence

import torch

from oracle import flux_oracle as orc


def active_steps(n: int, start: float, end: float):
    """diffusers' ``controlnet_keep`` (recalled): step i of n runs iff not (i / n < start or (i + 1) / n > end)."""
    return [i for i in range(n) if not (i / n < start or (i + 1) / n > end)]


def weights(sigmas, begin: int = 0, order: int = 2) -> List[float]:
    """w_i for i < n = len(sigmas) − 1; 0 up to and including ``begin`` and everywhere at order 1."""
    s = [float(x) for x in sigmas]
    out = []
    for i in range(len(s) - 1):
        first_order = order == 1 or i <= begin
        out.append(0.0 if first_order else (s[i + 1] - s[i]) / (2.0 * (s[i] - s[i - 1])))
    return out


def integrate(velocity: Callable, x, sigmas, begin: int = 0, order: int = 2):
    """x after the steps begin..n−1 of the rule with ``velocity(x, sigma)``."""
    s = [float(v) for v in sigmas]
    w = weights(s, begin, order)
    prev = None
    for i in range(begin, len(s) - 1):
        v = velocity(x, s[i])
        v2 = v if prev is None or w[i] == 0.0 else v + w[i] * (v - prev)
        x = x + (s[i + 1] - s[i]) * v2
        prev = v
    return x


def projected_velocity(p, u, r_prev, beta: float, s: float, eta: float, tau: float, dtype=torch.float64):
    """(v, d) of one guided step; p, u, r_prev [B, ...], the sums over everything but the leading dimension. ``r_prev`` None or
    ``beta`` 0: no momentum. The sums, k and α are always formed in float64; ``dtype`` is that of d and v (the loop uses float32)."""
    p, u = p.to(dtype), u.to(dtype)
    d = p - u
    if beta != 0.0 and r_prev is not None:
        d = d + beta * r_prev.to(dtype)
    dims = tuple(range(1, p.dim()))
    d64, p64 = d.double(), p.double()
    a, b, c = (d64 * d64).sum(dims, keepdim=True), (d64 * p64).sum(dims, keepdim=True), (p64 * p64).sum(dims, keepdim=True)
    one = torch.ones_like(a)
    k = torch.where((a > tau * tau) & (tau > 0), tau / torch.sqrt(torch.where(a > 0, a, one)), one)
    alpha = torch.where(c > 0, k * b / torch.where(c > 0, c, one), torch.zeros_like(c))
    e = (eta - 1.0) * alpha
    v = p + (float(s) - 1.0) * (k.to(dtype) * d + e.to(dtype) * p)
    return v, d


def denoise_loop_reference(tp, tcfg: dict, cp, ccfg: Optional[dict], latents, prompt_embeds, pooled, control_images: Sequence[torch.Tensor],
                           control_masks: Sequence[Optional[torch.Tensor]], sigmas, img_ids, txt_ids, guidance_scale: float,
                           conditioning_scale: float = 1.0, conditioning_step: int = 10 ** 9, *, negative: Optional[dict] = None,
                           union: Optional[dict] = None, repaint: Optional[dict] = None, order: int = 1, guider=None,
                           image_prompt: Optional[dict] = None, info: Optional[dict] = None):
    """The positional arguments of ``orc.denoise_loop``: latents [B,N,64]; control_images per text line [B,N,128]; control_masks per
    line [1,N,1], [B,N,1] or None; sigmas the FULL schedule with its trailing 0.

    negative      dict(prompt_embeds, pooled, scale): true CFG. The conditioning batch of a guided step is cat([negative, positive])
                  against latents of batch B, which the models see repeated; hints, the union hint and per-image masks are doubled the
                  same way, a shared [1,N,1] mask serves both halves. No zero-velocity first step: that is the inpaint flow's.
    union         dict(params, cfg, cond [B,N,64], scale, start, end): an unmasked tower, summed first, inside its interval. The samples
                  keep the text tower's depth (``ccfg``): a shallower union tower adds into the leading ones.
    repaint       dict(src, noise [B,N,64], mask [1 or B,N,64], t_start, blend=True): ``latents`` is ignored, the run walks
                  ``sigmas[t_start:]`` from the source re-noised to its first sigma, and every step ends with the blend unless ``blend``
                  is false (the plain loop from the same start).
    order         2: the multistep rule. Its history holds whatever velocity the step before used, guided or not.
    guider        any object with start, stop, eta, norm_threshold, momentum; needs ``negative``. Outside its interval the models run
                  on the positive half alone, at batch B; r_prev is carried from one guided step to the next.
    image_prompt  dict(forward, ip_params, ip_scales, embeds [B,E], neg_embeds [B,E]): ``forward`` is the ``transformer_forward`` of the
                  restatement (tests/ip_adapter_reference.py or tests/instantx_reference.py).
    info          a dict that receives ``norm_d`` (per projected step, the per-sample L2 norm of d).

    Steps — the union interval, the guider's interval and ``conditioning_step`` — are counted over the steps that run."""
    B = (repaint["src"] if repaint is not None else latents).shape[0]
    two = lambda t: torch.cat([t, t], dim=0)
    t_start = repaint["t_start"] if repaint is not None else 0
    w = weights(sigmas, t_start, order)[t_start:]
    sig = sigmas[t_start:]
    n = len(sig) - 1
    if repaint is not None:
        src, noise, blend_mask = repaint["src"].float(), repaint["noise"].float(), repaint["mask"]
        latents = (1.0 - float(sig[0])) * src + float(sig[0]) * noise
    if guider is not None:
        guided = set(active_steps(n, float(guider.start), float(guider.stop)))
    else:
        guided = set(range(n)) if negative is not None else set()
    projected = guider is not None and (guider.eta != 1 or guider.norm_threshold > 0 or guider.momentum != 0)
    if negative is not None:
        pe2 = torch.cat([negative["prompt_embeds"], prompt_embeds], dim=0)
        pl2 = torch.cat([negative["pooled"], pooled], dim=0)
    keep_union = set(active_steps(n, union["start"], union["end"])) if union is not None else set()
    forward = orc.transformer_forward if image_prompt is None else image_prompt["forward"]
    n_samples = ccfg["num_layers"] if ccfg is not None else 0
    hist = r_prev = None
    if info is not None:
        info["norm_d"] = []
    for i in range(n):
        on = i in guided
        rep = two if on else (lambda t: t)
        pe, pl = (pe2, pl2) if on else (prompt_embeds, pooled)
        lat_in = rep(latents)
        Bc = lat_in.shape[0]
        timestep = orc._model_t(sig[i] * 1000.0).expand(Bc)
        guidance = torch.full((Bc,), float(guidance_scale)) if tcfg.get("guidance_embeds", False) else None
        merged = [None] * n_samples

        def add(samples):
            for j, s in enumerate(samples):
                merged[j] = orc._s(s) if merged[j] is None else orc._s(merged[j] + s)

        if i in keep_union:
            us, _ = orc.controlnet_forward(union["params"], union["cfg"], lat_in, rep(union["cond"]), pe, pl, timestep, img_ids, txt_ids,
                                           guidance=guidance, conditioning_scale=union["scale"], _store_samples=False)
            add(us)
        if i < conditioning_step and cp is not None:
            for line, cond in enumerate(control_images):
                samples, _ = orc.controlnet_forward(cp, ccfg, lat_in, rep(cond), pe, pl, timestep, img_ids, txt_ids, guidance=guidance,
                                                    conditioning_scale=conditioning_scale, _store_samples=False)
                mask = control_masks[line] if len(control_masks) > 0 else None
                if mask is not None:
                    samples = [(mask if mask.shape[0] == 1 else rep(mask)) * s for s in samples]
                add(samples)
        if all(m is None for m in merged):
            block_samples = None
        else:
            zero = next(m for m in merged if m is not None) * 0.0
            block_samples = [zero if m is None else m for m in merged]
        fkw = {}
        if image_prompt is not None:
            embeds = image_prompt["embeds"]
            fkw = dict(ip_params=image_prompt["ip_params"], ip_scales=image_prompt["ip_scales"],
                       ip_embeds=torch.cat([image_prompt["neg_embeds"], embeds], dim=0) if on else embeds)
        v = forward(tp, tcfg, lat_in, pe, pl, timestep, img_ids, txt_ids, guidance=guidance, controlnet_block_samples=block_samples, **fkw)
        if not on:
            vel = v
        elif not projected:
            v_neg, v_pos = v[:B], v[B:]
            vel = v_neg + float(negative["scale"]) * (v_pos - v_neg)                 # fp32, not rounded under stored_as
        else:
            vel, r_prev = projected_velocity(v[B:], v[:B], r_prev, float(guider.momentum), float(negative["scale"]), float(guider.eta),
                                             float(guider.norm_threshold), dtype=torch.float32)
            if info is not None:
                info["norm_d"].append(r_prev.double().flatten(1).norm(dim=1))
        vel2 = vel if hist is None or w[i] == 0.0 else vel + w[i] * (vel - hist)
        hist = vel
        sn = float(sig[i + 1])
        r = orc.euler_step(latents, vel2, float(sig[i]), sn)
        if repaint is not None and repaint.get("blend", True):
            kept = (1.0 - sn) * src + sn * noise
            latents = (1.0 - blend_mask) * kept + blend_mask * r
        else:
            latents = r
    return latents
