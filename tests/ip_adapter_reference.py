"""fp32 CPU restatement of the IP-Adapter math for the tests (a plain helper module, not a conftest).

It imports oracle.flux_oracle for every primitive (linear, layer_norm, rms_norm, attention's rounding conventions, stored_as, the fp8
contexts) and restates ``double_block``, ``transformer_forward`` and the denoising loop with ONE term added:

    h <- h + s_i · softmax(q_i K_iᵀ / √128) V_i          after the block's feed-forward residual, image stream only,
    q_i = rms_norm(to_q(norm1(h))) · norm_q.weight        (after norm_q, before RoPE), K_i / V_i = to_k_ip_i / to_v_ip_i(tok),
    tok = LayerNorm_C(reshape(proj(embeds), [B, n, C]))   affine, eps 1e-5.

A block whose scale is 0 adds nothing (the term is skipped, as on the device), so with every scale 0 these functions compute exactly
what the oracle's do. Under ``orc.stored_as(bf16)`` the values the HIP path keeps as bf16 are rounded where it rounds them: the image
embeds, the tokens, K/V, the normalised query (the MFMA operand), the softmax numerators (row sums from the unrounded ones, as in
orc.attention) and the term itself. Adapter weights use the diffusers key layout.
"""
import math

import torch
import torch.nn.functional as F

from oracle import flux_oracle as orc


# --------------------------------------------------------------------------------------- the kernel's math on plain tensors
def ip_attention_ref(q, wq, k, v, ip_scale, sm_scale=128 ** -0.5, eps=1e-6, *, norm=True, weight=True, pad_keys_to=None, uniform=False):
    """fp32 reference of rt_ip_attention: q [B,N,H,128] raw, wq [128], k/v [B or 1,n,H,128] -> [B,N,H*128].
    The switches build the WRONG answers the tests use to prove that each step of the math is visible in their inputs:
    norm=False skips the RMSNorm, weight=False skips norm_q.weight, pad_keys_to=m appends zero keys/values up to m and leaves them
    unmasked (logit 0), uniform=True replaces the softmax by the mean over keys."""
    q, k, v = q.float(), k.float(), v.float()
    B, N, H, Dh = q.shape
    if norm:
        q = q * torch.rsqrt(q.pow(2).mean(-1, keepdim=True) + eps)
    if weight:
        q = q * wq.float()
    if pad_keys_to is not None and pad_keys_to > k.shape[1]:
        z = torch.zeros(k.shape[0], pad_keys_to - k.shape[1], H, Dh)
        k, v = torch.cat([k, z], dim=1), torch.cat([v, z], dim=1)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k.expand(B, -1, -1, -1)) * sm_scale
    p = torch.full_like(s, 1.0 / s.shape[-1]) if uniform else torch.softmax(s, dim=-1)
    o = torch.einsum("bhqk,bkhd->bqhd", p, v.expand(B, -1, -1, -1))
    return ip_scale * o.reshape(B, N, H * Dh)


# --------------------------------------------------------------------------------------- adapter weights
def init_ip_params(cfg, n_tokens, embed_dim, seed, kv_std=0.1, layout="diffusers"):
    """Random adapter (bf16-rounded, stored fp32) in the diffusers or the XLabs key layout. to_k_ip weights of std 0.1 give keys of
    std ≈ 1.6 (C = 256): logits far from flat, so a wrong K is visible at the model level."""
    g = torch.Generator().manual_seed(seed)
    C, d, L = cfg["joint_attention_dim"], cfg["num_attention_heads"] * cfg["attention_head_dim"], cfg["num_layers"]
    r = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(torch.bfloat16).float()
    pp, npfx = ("image_proj.proj", "image_proj.norm") if layout == "diffusers" else ("ip_adapter_proj_model.proj", "ip_adapter_proj_model.norm")
    p = {f"{pp}.weight": r(n_tokens * C, embed_dim, std=embed_dim ** -0.5), f"{pp}.bias": r(n_tokens * C, std=0.02),
         f"{npfx}.weight": (1.0 + 0.1 * torch.randn(C, generator=g)).to(torch.bfloat16).float(), f"{npfx}.bias": r(C, std=0.02)}
    for i in range(L):
        kk, vv = ((f"ip_adapter.{i}.to_k_ip", f"ip_adapter.{i}.to_v_ip") if layout == "diffusers" else
                  (f"double_blocks.{i}.processor.ip_adapter_double_stream_k_proj", f"double_blocks.{i}.processor.ip_adapter_double_stream_v_proj"))
        p[f"{kk}.weight"], p[f"{kk}.bias"] = r(d, C, std=kv_std), r(d, std=0.02)
        p[f"{vv}.weight"], p[f"{vv}.bias"] = r(d, C, std=0.05), r(d, std=0.02)
    return p


def to_xlabs(p):
    """The same tensors under the XLabs key names."""
    out = {}
    for k, v in p.items():
        k = k.replace("image_proj.", "ip_adapter_proj_model.")
        if k.startswith("ip_adapter."):
            _, i, which, part = k.split(".")
            k = f"double_blocks.{i}.processor.ip_adapter_double_stream_{which[3]}_proj.{part}"
        out[k] = v
    return out


def ip_tokens(ipp, embeds, C):
    """Step 1: [B or 1, E] (or [.., 1, E]) -> tok [B or 1, n, C]."""
    e = orc._s(embeds.float().reshape(embeds.shape[0], -1))
    t = F.linear(e, ipp["image_proj.proj.weight"], ipp["image_proj.proj.bias"]).reshape(e.shape[0], -1, C)
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return orc._s((t - mu) * torch.rsqrt(var + 1e-5) * ipp["image_proj.norm.weight"] + ipp["image_proj.norm.bias"])


def ip_kv(ipp, tok, i, H, Dh):
    """Step 2 for block i: (K_i, V_i) [B or 1, n, H, Dh]."""
    k = orc._s(F.linear(tok, ipp[f"ip_adapter.{i}.to_k_ip.weight"], ipp[f"ip_adapter.{i}.to_k_ip.bias"]))
    v = orc._s(F.linear(tok, ipp[f"ip_adapter.{i}.to_v_ip.weight"], ipp[f"ip_adapter.{i}.to_v_ip.bias"]))
    return k.reshape(*k.shape[:2], H, Dh), v.reshape(*v.shape[:2], H, Dh)


def ip_term(q_normed, k, v, scale):
    """Step 3 from the normalised query [B,N,H,Dh]: scale · softmax(q Kᵀ/√Dh) V -> [B,N,H*Dh], rounded where the kernel rounds."""
    B, N, H, Dh = q_normed.shape
    qh = orc._s(q_normed).permute(0, 2, 1, 3)
    kh, vh = (t.expand(B, -1, -1, -1).permute(0, 2, 1, 3) for t in (k, v))
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(Dh)
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = (orc._s(e) @ vh) / e.sum(dim=-1, keepdim=True)
    return orc._s(scale * o.permute(0, 2, 1, 3).reshape(B, N, H * Dh))


# --------------------------------------------------------------------------------------- blocks and models (restated from the oracle)
def double_block(p, pre, h, e, temb, rope, H=24, Dh=128, ip=None):
    """orc.double_block with ``ip`` = (K, V, scale) or None. Returns (e, h)."""
    linear, _s, _ln_out, _act_out = orc.linear, orc._s, orc._ln_out, orc._act_out
    layer_norm, rms_norm, silu, gelu_tanh, apply_rope = orc.layer_norm, orc.rms_norm, orc.silu, orc.gelu_tanh, orc.apply_rope
    T = e.shape[1]
    cos, sin = rope
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = linear(p, f"{pre}.norm1.linear", silu(temb)).chunk(6, dim=-1)
    csh_a, csc_a, cg_a, csh_m, csc_m, cg_m = linear(p, f"{pre}.norm1_context.linear", silu(temb)).chunk(6, dim=-1)
    nh = _ln_out(layer_norm(h) * (1 + sc_a[:, None]) + sh_a[:, None])
    ne = _ln_out(layer_norm(e) * (1 + csc_a[:, None]) + csh_a[:, None])

    def heads(x):
        return _s(x).reshape(x.shape[0], x.shape[1], H, Dh)

    q = rms_norm(heads(linear(p, f"{pre}.attn.to_q", nh)), p[f"{pre}.attn.norm_q.weight"])
    k = rms_norm(heads(linear(p, f"{pre}.attn.to_k", nh)), p[f"{pre}.attn.norm_k.weight"])
    v = heads(linear(p, f"{pre}.attn.to_v", nh))
    eq = rms_norm(heads(linear(p, f"{pre}.attn.add_q_proj", ne)), p[f"{pre}.attn.norm_added_q.weight"])
    ek = rms_norm(heads(linear(p, f"{pre}.attn.add_k_proj", ne)), p[f"{pre}.attn.norm_added_k.weight"])
    ev = heads(linear(p, f"{pre}.attn.add_v_proj", ne))
    Q = _s(apply_rope(torch.cat([eq, q], dim=1), cos, sin))   # text first
    K = _s(apply_rope(torch.cat([ek, k], dim=1), cos, sin))
    V = torch.cat([ev, v], dim=1)
    A = orc.attention(Q, K, V)
    a_e = linear(p, f"{pre}.attn.to_add_out", A[:, :T])
    a_h = linear(p, f"{pre}.attn.to_out.0", A[:, T:])

    def ff(name, x):
        return linear(p, f"{pre}.{name}.net.2", _act_out(gelu_tanh(linear(p, f"{pre}.{name}.net.0.proj", x))))

    h = h + g_a[:, None] * a_h
    h = h + g_m[:, None] * ff("ff", _ln_out(layer_norm(h) * (1 + sc_m[:, None]) + sh_m[:, None]))
    if ip is not None and ip[2] != 0.0:
        h = h + ip_term(q, ip[0], ip[1], ip[2])               # the added term: q after norm_q, before RoPE
    e = e + cg_a[:, None] * a_e
    e = e + cg_m[:, None] * ff("ff_context", _ln_out(layer_norm(e) * (1 + csc_m[:, None]) + csh_m[:, None]))
    return e, h


def transformer_forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                        controlnet_block_samples=None, controlnet_single_block_samples=None, ip_params=None, ip_embeds=None, ip_scales=None):
    """orc.transformer_forward with the adapter (ip_params in the diffusers layout, ip_embeds [B or 1, E], ip_scales per block)."""
    linear, _s = orc.linear, orc._s
    H, Dh = cfg["num_attention_heads"], cfg["attention_head_dim"]
    h = linear(p, "x_embedder", _s(hidden_states))
    t1000 = orc._x1000(timestep)
    g1000 = orc._x1000(guidance) if (guidance is not None and cfg.get("guidance_embeds", False)) else None
    temb = orc.time_text_embed(p, "time_text_embed", t1000, g1000, pooled_projections)
    e = linear(p, "context_embedder", _s(encoder_hidden_states))
    rope = orc.rope_table(torch.cat([txt_ids, img_ids], dim=0).float(), cfg.get("axes_dims_rope", (16, 56, 56)))
    nl, ns = cfg["num_layers"], cfg["num_single_layers"]
    tok = None
    if ip_params is not None and ip_embeds is not None and any(s != 0.0 for s in ip_scales):
        tok = ip_tokens(ip_params, ip_embeds, cfg["joint_attention_dim"])
    for i in range(nl):
        ip = None
        if tok is not None and ip_scales[i] != 0.0:
            ip = (*ip_kv(ip_params, tok, i, H, Dh), float(ip_scales[i]))
        e, h = double_block(p, f"transformer_blocks.{i}", h, e, temb, rope, H, Dh, ip=ip)
        if controlnet_block_samples is not None:
            k = int(math.ceil(nl / len(controlnet_block_samples)))
            h = h + controlnet_block_samples[i // k]
    T = e.shape[1]
    x = torch.cat([e, h], dim=1)
    for i in range(ns):
        x = orc.single_block(p, f"single_transformer_blocks.{i}", x, temb, rope, H, Dh)
        if controlnet_single_block_samples is not None:
            k = int(math.ceil(ns / len(controlnet_single_block_samples)))
            x = torch.cat([x[:, :T], x[:, T:] + controlnet_single_block_samples[i // k]], dim=1)
    h = x[:, T:]
    scale, shift = linear(p, "norm_out.linear", orc.silu(temb)).chunk(2, dim=-1)
    h = _s(orc.layer_norm(h) * (1 + scale[:, None]) + shift[:, None])
    return _s(linear(p, "proj_out", h))


def denoise_loop(tp, tcfg, cp, ccfg, latents, prompt_embeds, pooled, control_images, control_masks, sigmas, img_ids, txt_ids,
                 guidance_scale, conditioning_scale=1.0, conditioning_step=10 ** 9, ip_params=None, ip_embeds=None, ip_scales=None):
    """orc.denoise_loop (text-to-image) with the adapter in the transformer; the towers are untouched."""
    _s = orc._s
    B = latents.shape[0]
    n = len(sigmas) - 1
    for i in range(n):
        t = sigmas[i] * 1000.0
        timestep = orc._model_t(t).expand(B)
        guidance = torch.full((B,), float(guidance_scale)) if tcfg.get("guidance_embeds", False) else None
        merged = None
        for line, cond in enumerate(control_images):
            if i < conditioning_step and cp is not None:
                samples, _ = orc.controlnet_forward(cp, ccfg, latents, cond, prompt_embeds, pooled, timestep, img_ids, txt_ids,
                                                    guidance=guidance, conditioning_scale=conditioning_scale, _store_samples=False)
            else:
                samples = None
            if samples is not None:
                mask = control_masks[line] if len(control_masks) > 0 else None
                if mask is not None:
                    samples = [mask * s for s in samples]
            if line == 0:
                merged = None if samples is None else [_s(a) for a in samples]
            elif samples is not None and merged is not None:
                merged = [_s(a + b) for a, b in zip(merged, samples)]
        v = transformer_forward(tp, tcfg, latents, prompt_embeds, pooled, timestep, img_ids, txt_ids, guidance=guidance,
                                controlnet_block_samples=merged, ip_params=ip_params, ip_embeds=ip_embeds, ip_scales=ip_scales)
        latents = orc.euler_step(latents, v, float(sigmas[i]), float(sigmas[i + 1]))
    return latents
