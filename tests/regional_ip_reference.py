"""fp32 CPU restatement of regional image prompts for the tests (a plain helper module, not a conftest): the blocks of
tests/ip_adapter_reference.py (XLabs / diffusers form) and tests/instantx_reference.py (InstantX form) with a LIST of weighted terms.

A term is dict(embeds [B or 1, E], neg_embeds [B or 1, E] or None, mask [1 or B, N, 1] or None, scale, line):

    image row n of batch entry b weighs   w[b, n] = scale · mask[b, n]               (mask None: the call's own prompt, unweighted)
    the T text rows of an InstantX single block all weigh   scale · mean_n mask[b, n]
    under true CFG the conditioning batch is [negative, positive]: the call's own prompt (line False) uses neg_embeds under the same
    mask in the negative half; a text line's term weighs 0 there.

Terms add in order, each into the place the single term goes, with the rounding the HIP path has there under ``orc.stored_as``: the
XLabs term waits in a bf16 buffer (first term written, each later one added with one more rounding) and is added after the feed-forward
residual; the InstantX double-block terms go onto the fp32 residual one after another, gated and unrounded; the InstantX single-block
terms wait in a bf16 buffer like the XLabs ones and are added to the bf16 attention output."""
import contextlib
import math

import torch

import instantx_reference as ixr
import ip_adapter_reference as ipr
import line_prompt_reference as lpr
from oracle import flux_oracle as orc


def term_tables(term, B, Bc, T):
    """(embeds [Bc, E], image weights [Bc, N, 1] or None, joint weights [Bc, T + N, 1] or None) of a term at conditioning batch Bc."""
    e = term["embeds"].float().expand(B, -1)
    m = term.get("mask")
    wi = wj = None
    if m is not None:
        m = m.float().expand(B, -1, -1)
        wi = float(term["scale"]) * m
        wt = float(term["scale"]) * m.mean(dim=1, keepdim=True)
    if Bc == 2 * B:
        neg = term.get("neg_embeds")
        e = torch.cat([e if neg is None else neg.float().expand(B, -1), e])
        if wi is not None:
            off = 0.0 if term.get("line") else 1.0
            wi, wt = torch.cat([off * wi, wi]), torch.cat([off * wt, wt])
    if wi is not None:
        wj = torch.cat([wt.expand(-1, T, -1), wi], dim=1)
    return e, wi, wj


def _buffer(parts):
    """Terms that wait in one bf16 buffer: the first written, each later one added with one more rounding."""
    buf = None
    for t in parts:
        buf = orc._s(t) if buf is None else orc._s(buf + t)
    return buf


def _weighted(o, scale, w):
    return scale * o if w is None else (scale * w) * o


def double_block(p, pre, h, e, temb, rope, H, Dh, terms, inside):
    """orc.double_block with ``terms`` = [(K, V, scale, w [B,N,1] or None)]. Returns (e, h)."""
    linear, _s, _ln_out, _act_out = orc.linear, orc._s, orc._ln_out, orc._act_out
    layer_norm, rms_norm, silu, gelu_tanh, apply_rope = orc.layer_norm, orc.rms_norm, orc.silu, orc.gelu_tanh, orc.apply_rope
    T = e.shape[1]
    cos, sin = rope
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = linear(p, f"{pre}.norm1.linear", silu(temb)).chunk(6, dim=-1)
    csh_a, csc_a, cg_a, csh_m, csc_m, cg_m = linear(p, f"{pre}.norm1_context.linear", silu(temb)).chunk(6, dim=-1)
    nh = _ln_out(layer_norm(h) * (1 + sc_a[:, None]) + sh_a[:, None])
    ne = _ln_out(layer_norm(e) * (1 + csc_a[:, None]) + csh_a[:, None])
    heads = lambda x: _s(x).reshape(x.shape[0], x.shape[1], H, Dh)
    q = rms_norm(heads(linear(p, f"{pre}.attn.to_q", nh)), p[f"{pre}.attn.norm_q.weight"])
    k = rms_norm(heads(linear(p, f"{pre}.attn.to_k", nh)), p[f"{pre}.attn.norm_k.weight"])
    v = heads(linear(p, f"{pre}.attn.to_v", nh))
    eq = rms_norm(heads(linear(p, f"{pre}.attn.add_q_proj", ne)), p[f"{pre}.attn.norm_added_q.weight"])
    ek = rms_norm(heads(linear(p, f"{pre}.attn.add_k_proj", ne)), p[f"{pre}.attn.norm_added_k.weight"])
    ev = heads(linear(p, f"{pre}.attn.add_v_proj", ne))
    Q = _s(apply_rope(torch.cat([eq, q], dim=1), cos, sin))
    K = _s(apply_rope(torch.cat([ek, k], dim=1), cos, sin))
    A = orc.attention(Q, K, torch.cat([ev, v], dim=1))
    a_e = linear(p, f"{pre}.attn.to_add_out", A[:, :T])
    a_h = linear(p, f"{pre}.attn.to_out.0", A[:, T:])
    ff = lambda name, x: linear(p, f"{pre}.{name}.net.2", _act_out(gelu_tanh(linear(p, f"{pre}.{name}.net.0.proj", x))))
    if inside:
        for Kt, Vt, s, w in terms:                            # gated, onto the fp32 residual, before the attention's, in order
            h = h + g_a[:, None] * _weighted(ixr.ix_attn(q, Kt, Vt), s, w)
    h = h + g_a[:, None] * a_h
    h = h + g_m[:, None] * ff("ff", _ln_out(layer_norm(h) * (1 + sc_m[:, None]) + sh_m[:, None]))
    if not inside and terms:
        h = h + _buffer([_weighted(ixr.ix_attn(q, Kt, Vt), s, w) for Kt, Vt, s, w in terms])
    e = e + cg_a[:, None] * a_e
    e = e + cg_m[:, None] * ff("ff_context", _ln_out(layer_norm(e) * (1 + csc_m[:, None]) + csh_m[:, None]))
    return e, h


def single_block(p, pre, x, temb, rope, H, Dh, terms):
    """orc.single_block with ``terms`` = [(K, V, scale, w [B,S,1] or None)] (the InstantX form)."""
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
    if terms:
        A = _s(_s(A) + _buffer([_weighted(ixr.ix_attn(q, Kt, Vt), s, w) for Kt, Vt, s, w in terms]))
    return x + g[:, None] * linear(p, f"{pre}.proj_out", torch.cat([A, m], dim=2))


def transformer_forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                        controlnet_block_samples=None, *, ip_params, ip_scales, terms, layout, B=None):
    """orc.transformer_forward with the weighted terms. ``layout`` "instantx" or "diffusers" (ip_params in that layout); ``B`` the
    latents' batch when hidden_states already holds [negative, positive] (default: hidden_states' own batch)."""
    linear, _s = orc.linear, orc._s
    H, Dh, C = cfg["num_attention_heads"], cfg["attention_head_dim"], cfg["joint_attention_dim"]
    inside = layout == "instantx"
    Bc = hidden_states.shape[0]
    T = encoder_hidden_states.shape[1]
    h = linear(p, "x_embedder", _s(hidden_states))
    t1000 = orc._x1000(timestep)
    g1000 = orc._x1000(guidance) if (guidance is not None and cfg.get("guidance_embeds", False)) else None
    temb = orc.time_text_embed(p, "time_text_embed", t1000, g1000, pooled_projections)
    e = linear(p, "context_embedder", _s(encoder_hidden_states))
    rope = orc.rope_table(torch.cat([txt_ids, img_ids], dim=0).float(), cfg.get("axes_dims_rope", (16, 56, 56)))
    nl, ns = cfg["num_layers"], cfg["num_single_layers"]
    tabs = [term_tables(t, B or Bc, Bc, T) for t in terms] if any(s != 0.0 for s in ip_scales) else []
    toks = [(ixr.ix_tokens if inside else ipr.ip_tokens)(ip_params, em, C) for em, _, _ in tabs]

    def terms_of(j, single=False):
        if ip_scales[j] == 0.0:
            return []
        kv = ixr.ix_kv if inside else ipr.ip_kv
        return [(*kv(ip_params, tok, j, H, Dh), float(ip_scales[j]), wj if single else wi) for tok, (_, wi, wj) in zip(toks, tabs)]

    for i in range(nl):
        e, h = double_block(p, f"transformer_blocks.{i}", h, e, temb, rope, H, Dh, terms_of(i), inside)
        if controlnet_block_samples is not None:
            k = int(math.ceil(nl / len(controlnet_block_samples)))
            h = h + controlnet_block_samples[i // k]
    x = torch.cat([e, h], dim=1)
    for i in range(ns):
        x = single_block(p, f"single_transformer_blocks.{i}", x, temb, rope, H, Dh, terms_of(nl + i, single=True) if inside else [])
    h = x[:, T:]
    scale, shift = linear(p, "norm_out.linear", orc.silu(temb)).chunk(2, dim=-1)
    h = _s(orc.layer_norm(h) * (1 + scale[:, None]) + shift[:, None])
    return _s(linear(p, "proj_out", h))


def image_prompt_slot(ip_params, ip_scales, terms, layout, B, lines=None):
    """What loop_reference.denoise_loop_reference(image_prompt=) takes. ``lines`` = (line_embeds [B, R·L, D], ends, row_vis [B or 2B, S]):
    per-line prompts too, the text stream and the attention mask of tests/line_prompt_reference.py."""
    def forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                controlnet_block_samples=None, **unused):
        Bc = hidden_states.shape[0]
        ctx = contextlib.nullcontext()
        if lines is not None:
            le, ends, row_vis = lines
            le = le if Bc == le.shape[0] else torch.cat([le, le], dim=0)
            encoder_hidden_states = torch.cat([encoder_hidden_states, le], dim=1)
            txt_ids = torch.zeros(encoder_hidden_states.shape[1], 3)
            ctx = lpr.attention_as(lpr.masked_attention(lpr.visible(ends, row_vis[-Bc:])))
        with ctx:
            return transformer_forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids,
                                       guidance=guidance, controlnet_block_samples=controlnet_block_samples, ip_params=ip_params,
                                       ip_scales=ip_scales, terms=terms, layout=layout, B=B)
    z = torch.zeros(B, 1)
    return dict(forward=forward, ip_params=None, ip_scales=None, embeds=z, neg_embeds=z)
