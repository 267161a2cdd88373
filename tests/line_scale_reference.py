"""fp32 CPU restatement of a strength per line prompt (``control_prompt_scale``) for the tests (a plain helper module, not a conftest).

The transformer's joint attention is ``line_prompt_reference.masked_attention`` — the oracle's, with -inf on the hidden keys — with one more
term in the logits:

    logit(i, j) = q_i . k_j / sqrt(Dh) + ln w(j),    w(j) = the scale of the line prompt that key j is a token of, 1 for every other key

and that function's rounding points under ``orc.stored_as``: the row sums come from the unrounded numerators, the numerators are rounded
as the second product's operand, the output is rounded once. The rule is restated here from the text layout (``key_log_scale``), not
imported from the package: keys [T0 + (r - 1) L, T0 + r L) are line r's. Everything else is the oracle's own forward and loop."""
import math

import torch

from oracle import flux_oracle as orc

import line_prompt_reference as lpr


def key_log_scale(T0, L, scales, S):
    """fp32 [S]: ln w on the L tokens of each line prompt (``scales``: one per line THAT HAS A PROMPT, in order), 0 elsewhere."""
    out = torch.zeros(S, dtype=torch.float32)
    for r, w in enumerate(scales):
        out[T0 + r * L : T0 + (r + 1) * L] = math.log(w)
    return out


def biased_attention(see, key_bias):
    """lpr.masked_attention with key_bias[j] added to the logits of key j. see: bool [B or 1, S, S]; key_bias: fp32 [S]."""
    def attention(q, k, v):
        B, S, H, Dh = q.shape
        qh, kh, vh = (t.permute(0, 2, 1, 3) for t in (q, k, v))
        s = (qh @ kh.transpose(-1, -2)) / math.sqrt(Dh) + key_bias.to(q.dtype)[None, None, None, :]
        s = s.masked_fill(~see[:, None].expand(B, H, S, S), float("-inf"))
        if orc._STORE is None:
            o = torch.softmax(s, dim=-1) @ vh
        else:
            e = torch.exp(s - s.amax(dim=-1, keepdim=True))
            o = (orc._s(e) @ vh) / e.sum(dim=-1, keepdim=True)
        return orc._s(o.permute(0, 2, 1, 3).reshape(B, S, H * Dh))
    return attention


def forward_under(see, key_bias):
    """orc.transformer_forward on cat([prompt, line embeddings]) with the masked, biased softmax of (``see`` [B, S, S], ``key_bias`` [S])."""
    def forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                controlnet_block_samples=None, line_embeds=None, **unused):
        pe = torch.cat([encoder_hidden_states, line_embeds], dim=1)
        with lpr.attention_as(biased_attention(see[-hidden_states.shape[0]:], key_bias)):
            return orc.transformer_forward(p, cfg, hidden_states, pe, pooled_projections, timestep, img_ids, torch.zeros(pe.shape[1], 3),
                                           guidance=guidance, controlnet_block_samples=controlnet_block_samples)
    return forward


def loop_slot(line_embeds, see, key_bias):
    """denoise_loop_reference(image_prompt=): the forward above on the rows of ``see`` that belong to the batch it is called with
    ([negative, positive] at 2B, the positive half at B); the towers never see a line prompt."""
    def forward(p, cfg, hidden_states, *args, **kw):
        Bc = hidden_states.shape[0]
        le = line_embeds if Bc == line_embeds.shape[0] else torch.cat([line_embeds, line_embeds], dim=0)
        return forward_under(see, key_bias)(p, cfg, hidden_states, *args, line_embeds=le, **kw)
    z = torch.zeros(line_embeds.shape[0], 1)
    return dict(forward=forward, ip_params=None, ip_scales=None, embeds=z, neg_embeds=z)
