"""fp32 CPU restatement of the InstantX IP-Adapter math for the tests (a plain helper module, not a conftest).

Rules 1-5 of reptext_amd/ip_adapter.py's docstring on oracle.flux_oracle primitives, with the term inserted where rule 4 says:

    tok  = LayerNorm_C(reshape(proj.2(gelu_erf(proj.0(embeds))), [B, n, C]))          affine, eps 1e-5
    K_j  = rmsnorm_128(to_k_ip_j(tok))  (eps 1e-5, no weight),  V_j = to_v_ip_j(tok)    no bias, j over double blocks, then single blocks
    ip_j = softmax(q̂ K_jᵀ / √128) V_j                                                  q̂ after norm_q, before RoPE
    double block:  h <- h + gate_msa · (s_j · ip_j),  then  h <- h + gate_msa · to_out(attn_img)     (the order the device launches)
    single block:  x <- x + gate · proj_out([attn + s_j · ip_j | gelu(mlp)])                        q̂ = all S rows, text included

A block whose scale is 0 adds nothing, so with every scale 0 these functions compute exactly what the oracle's do. Under
``orc.stored_as(bf16)`` the values the HIP path keeps as bf16 are rounded where it rounds them: the embeds, the GELU hidden, the tokens,
the normalised K, V, q̂ (the MFMA operand), the softmax numerators (row sums from the unrounded ones, as in orc.attention) and, in
single blocks, the term and its sum with the attention output. A double block's term goes onto the fp32 residual unrounded.

``variant`` builds the WRONG answers the tests use to show that a rule is visible in their inputs: "no_text_rows" leaves the text rows
of single blocks out of the term, "ungated" adds the double-block term without gate_msa.
"""
import math

import torch
import torch.nn.functional as F

from oracle import flux_oracle as orc

SMALL_T = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=4,
               joint_attention_dim=256, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
SMALL_CN = dict(SMALL_T, num_layers=2, num_single_layers=0, extra_condition_channels=64)
E = 64


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# --------------------------------------------------------------------------------------- adapter weights
def init_instantx_params(cfg, n_tokens, embed_dim, seed, kv_std=0.1, v_std=0.05):
    """Random adapter (bf16-rounded, stored fp32) in the flat InstantX key layout: L2 + L1 bias-free K/V pairs."""
    g = torch.Generator().manual_seed(seed)
    C, d = cfg["joint_attention_dim"], cfg["num_attention_heads"] * cfg["attention_head_dim"]
    L = cfg["num_layers"] + cfg["num_single_layers"]
    r = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(torch.bfloat16).float()
    Ee = embed_dim
    p = {"image_proj.proj.0.weight": r(2 * Ee, Ee, std=Ee ** -0.5), "image_proj.proj.0.bias": r(2 * Ee, std=0.1),
         "image_proj.proj.2.weight": r(n_tokens * C, 2 * Ee, std=(Ee / 2) ** -0.5), "image_proj.proj.2.bias": r(n_tokens * C, std=0.02),
         "image_proj.norm.weight": (1.0 + 0.1 * torch.randn(C, generator=g)).to(torch.bfloat16).float(), "image_proj.norm.bias": r(C, std=0.02)}
    for j in range(L):
        p[f"ip_adapter.{j}.to_k_ip.weight"] = r(d, C, std=kv_std)
        p[f"ip_adapter.{j}.to_v_ip.weight"] = r(d, C, std=v_std)
    return p


def to_nested(p):
    """The same tensors in the upstream file form: {"image_proj": {...}, "ip_adapter": {...}} (what torch.save writes as ip-adapter.bin)."""
    out = {"image_proj": {}, "ip_adapter": {}}
    for k, v in p.items():
        pre, rest = k.split(".", 1)
        out[pre][rest] = v
    return out


# --------------------------------------------------------------------------------------- rules 1-3
def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ix_tokens(ipp, embeds, C):
    """Rule 1: [B or 1, E] (or [.., 1, E]) -> tok [B or 1, n, C]."""
    e = orc._s(embeds.float().reshape(embeds.shape[0], -1))
    hid = orc._s(gelu_erf(F.linear(e, ipp["image_proj.proj.0.weight"], ipp["image_proj.proj.0.bias"])))
    t = F.linear(hid, ipp["image_proj.proj.2.weight"], ipp["image_proj.proj.2.bias"]).reshape(e.shape[0], -1, C)
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return orc._s((t - mu) * torch.rsqrt(var + 1e-5) * ipp["image_proj.norm.weight"] + ipp["image_proj.norm.bias"])


def ix_kv(ipp, tok, j, H, Dh):
    """Rule 2 for block j: (K_j, V_j) [B or 1, n, H, Dh]; K normalised per head in fp32, then stored."""
    k = F.linear(tok, ipp[f"ip_adapter.{j}.to_k_ip.weight"]).reshape(*tok.shape[:2], H, Dh)
    k = orc._s(k * torch.rsqrt(k.pow(2).mean(-1, keepdim=True) + 1e-5))
    v = orc._s(F.linear(tok, ipp[f"ip_adapter.{j}.to_v_ip.weight"])).reshape(*tok.shape[:2], H, Dh)
    return k, v


def ix_attn(q_normed, k, v):
    """Rule 3 from the normalised query [B,R,H,Dh]: softmax(q̂ Kᵀ/√Dh) V -> fp32 [B,R,H*Dh] (q̂ and the numerators rounded as stored)."""
    B, R, H, Dh = q_normed.shape
    qh = orc._s(q_normed).permute(0, 2, 1, 3)
    kh, vh = (t.expand(B, -1, -1, -1).permute(0, 2, 1, 3) for t in (k, v))
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(Dh)
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = (orc._s(e) @ vh) / e.sum(dim=-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B, R, H * Dh)


def ip_attention_gated_ref(q, wq, k, v, ip_scale, gate=None, sm_scale=128 ** -0.5, eps=1e-6):
    """fp32 reference of rt_ip_attention_gated on plain tensors: q [B,R,H,128] raw, wq [128], k/v [B or 1,n,H,128], gate [B,H*128] or None."""
    q = q.float()
    B, R, H, Dh = q.shape
    qn = q * torch.rsqrt(q.pow(2).mean(-1, keepdim=True) + eps) * wq.float()
    s = torch.einsum("bqhd,bkhd->bhqk", qn, k.float().expand(B, -1, -1, -1)) * sm_scale
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v.float().expand(B, -1, -1, -1)).reshape(B, R, H * Dh) * ip_scale
    return o if gate is None else o * gate.float()[:, None]


# --------------------------------------------------------------------------------------- blocks and models (restated from the oracle)
def double_block(p, pre, h, e, temb, rope, H=24, Dh=128, ip=None, variant=None):
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

    if ip is not None and ip[2] != 0.0:                       # the added term: gated, onto the fp32 residual, before the attention's
        term = ip[2] * ix_attn(q, ip[0], ip[1])
        h = h + (term if variant == "ungated" else g_a[:, None] * term)
    h = h + g_a[:, None] * a_h
    h = h + g_m[:, None] * ff("ff", _ln_out(layer_norm(h) * (1 + sc_m[:, None]) + sh_m[:, None]))
    e = e + cg_a[:, None] * a_e
    e = e + cg_m[:, None] * ff("ff_context", _ln_out(layer_norm(e) * (1 + csc_m[:, None]) + csh_m[:, None]))
    return e, h


def single_block(p, pre, x, temb, rope, H=24, Dh=128, ip=None, T=0, variant=None):
    """orc.single_block with ``ip`` = (K, V, scale) or None; T = number of text rows (only the "no_text_rows" variant looks at it)."""
    linear, _s = orc.linear, orc._s
    B, S, d = x.shape
    cos, sin = rope
    sh, sc, g = linear(p, f"{pre}.norm.linear", orc.silu(temb)).chunk(3, dim=-1)
    nx = orc._ln_out(orc.layer_norm(x) * (1 + sc[:, None]) + sh[:, None])
    m = orc._act_out(orc.gelu_tanh(linear(p, f"{pre}.proj_mlp", nx)))
    q = orc.rms_norm(_s(linear(p, f"{pre}.attn.to_q", nx)).reshape(B, S, H, Dh), p[f"{pre}.attn.norm_q.weight"])
    k = orc.rms_norm(_s(linear(p, f"{pre}.attn.to_k", nx)).reshape(B, S, H, Dh), p[f"{pre}.attn.norm_k.weight"])
    v = _s(linear(p, f"{pre}.attn.to_v", nx)).reshape(B, S, H, Dh)
    A = orc.attention(_s(orc.apply_rope(q, cos, sin)), _s(orc.apply_rope(k, cos, sin)), v)
    if ip is not None and ip[2] != 0.0:
        term = _s(ip[2] * ix_attn(q, ip[0], ip[1]))           # the bf16 buffer the term waits in
        if variant == "no_text_rows":
            term = torch.cat([torch.zeros_like(term[:, :T]), term[:, T:]], dim=1)
        A = _s(_s(A) + term)                                  # a block with the adapter always has a bf16 attention output to add to
    return x + g[:, None] * linear(p, f"{pre}.proj_out", torch.cat([A, m], dim=2))


def transformer_forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                        controlnet_block_samples=None, controlnet_single_block_samples=None, ip_params=None, ip_embeds=None, ip_scales=None,
                        variant=None):
    """orc.transformer_forward with the InstantX adapter (ip_params flat, ip_embeds [B or 1, E], ip_scales per block, double first)."""
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
        tok = ix_tokens(ip_params, ip_embeds, cfg["joint_attention_dim"])

    def ip_of(j):
        if tok is None or ip_scales[j] == 0.0:
            return None
        return (*ix_kv(ip_params, tok, j, H, Dh), float(ip_scales[j]))

    for i in range(nl):
        e, h = double_block(p, f"transformer_blocks.{i}", h, e, temb, rope, H, Dh, ip=ip_of(i), variant=variant)
        if controlnet_block_samples is not None:
            k = int(math.ceil(nl / len(controlnet_block_samples)))
            h = h + controlnet_block_samples[i // k]
    T = e.shape[1]
    x = torch.cat([e, h], dim=1)
    for i in range(ns):
        x = single_block(p, f"single_transformer_blocks.{i}", x, temb, rope, H, Dh, ip=ip_of(nl + i), T=T, variant=variant)
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


# --------------------------------------------------------------------------------------- the model case both test files use
# The text rows of a single block reach the output (image rows only) through the attention of a LATER single block alone, so the
# active single block is the first one and the 0 sits on the last. To make that path >= 10 x the bf16 floor at 2 + 2 blocks the
# inputs are small (latents, prompt and ControlNet samples x 0.01): the residual stream is then made by the blocks themselves and a
# changed text row is a changed key/value, not a perturbation of a large residual. N = 81 image rows keeps the 64 text rows a large
# share of the keys. V weights of std 0.5 make the term as large as the attention output it is added to.
MODEL_SCALES = [0.0, 0.3, -1.0, 0.0]          # a 0 on one double and on one single block
MODEL_SEED = 410
MODEL_V_STD = 0.5
MODEL_INPUT_SCALE = 0.01


def model_inputs(B, seed, T=64, h2=18, w2=18, scale=MODEL_INPUT_SCALE):
    """N = (h2/2)·(w2/2) image rows (81: not a multiple of 64, S = 145: two workgroups of the kernel), T = 64, per-sample embeds."""
    g = torch.Generator().manual_seed(seed)
    N = (h2 // 2) * (w2 // 2)
    r = lambda *s, m=1.0: (torch.randn(*s, generator=g) * m).to(torch.bfloat16).float()
    return dict(latents=r(B, N, 64, m=scale), prompt=r(B, T, 256, m=scale), pooled=r(B, 64), img_ids=orc.latent_image_ids(h2, w2),
                txt_ids=torch.zeros(T, 3), timestep=torch.full((B,), 0.622459), guidance=torch.full((B,), 3.5),
                samples=[r(B, N, 512, m=0.5 * scale), r(B, N, 512, m=0.5 * scale)], embeds=r(B, E))


def model_case(n_tokens=16, seed=MODEL_SEED, B=2, samples=True, h2=18, w2=18, scales=None):
    """(transformer params, adapter params, inputs, oracle positional args, oracle kwargs, adapter kwargs) of the model-level tests."""
    tp = orc.init_mmdit_params(SMALL_T, seed=seed)
    ipp = init_instantx_params(SMALL_T, n_tokens=n_tokens, embed_dim=E, seed=seed + 1, v_std=MODEL_V_STD)
    x = model_inputs(B, seed + 2, h2=h2, w2=w2)
    targs = (tp, SMALL_T, x["latents"], x["prompt"], x["pooled"], x["timestep"], x["img_ids"], x["txt_ids"])
    okw = dict(guidance=x["guidance"], controlnet_block_samples=x["samples"] if samples else None)
    ikw = dict(ip_params=ipp, ip_embeds=x["embeds"], ip_scales=MODEL_SCALES if scales is None else scales)
    return tp, ipp, x, targs, okw, ikw
