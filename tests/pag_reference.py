"""fp32 CPU restatement of perturbed-attention guidance (``pag_scale`` / ``pag_applied_layers``) for the tests (a plain helper module, not
a conftest).

At a guided step the conditioning batch is [perturbed, positive]: both halves are the positive conditioning, and in the APPLIED blocks of
the transformer the first half's joint attention is the oracle's with -inf on the hidden keys,

    a text row sees every key;  image row i sees the T text keys and key i          (``perturbed_visible``)

restated here from the token layout (text rows first), not imported from the package. The step then mixes the halves as true CFG does
with s = 1 + pag_scale: v = u + s·(p − u) = p + pag_scale·(p − u), which is ``loop_reference.denoise_loop_reference``'s ``negative`` slot
with the positive embeddings in it. Every other block, the towers, and a guider's unguided steps (the positive half at batch B) run the
oracle's own attention.

``orc.transformer_forward`` calls ``orc.attention`` once per block, the double blocks first: ``applied_attention`` counts the calls of one
forward to know which block it is in, and keeps ``line_prompt_reference.masked_attention``'s rounding points under ``orc.stored_as``."""
import torch

from oracle import flux_oracle as orc

import line_prompt_reference as lpr


def perturbed_visible(T, N, B):
    """bool [2B, S, S] for the batch [perturbed, positive]."""
    S = T + N
    see = torch.ones(2 * B, S, S, dtype=torch.bool)
    see[:B, T:, T:] = torch.eye(N, dtype=torch.bool)
    return see


def applied_attention(see, n_double, double_ids, single_ids):
    """The attention of one transformer forward: ``lpr.masked_attention(see)`` in the applied blocks, the oracle's own in the others."""
    plain, masked = orc.attention, lpr.masked_attention(see)
    calls = [0]

    def attention(q, k, v):
        c = calls[0]
        calls[0] += 1
        on = (c in double_ids) if c < n_double else (c - n_double in single_ids)
        return masked(q, k, v) if on else plain(q, k, v)
    return attention


def forward_under(T, double_ids, single_ids):
    """A ``transformer_forward`` for the batch [perturbed, positive] (2B rows against ``B`` = half of them). Called with another batch
    than an even one it would be wrong: the loop slot below decides."""
    def forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                controlnet_block_samples=None, **unused):
        Bc, N = hidden_states.shape[0], hidden_states.shape[1]
        see = perturbed_visible(T, N, Bc // 2)
        with lpr.attention_as(applied_attention(see, cfg["num_layers"], frozenset(double_ids), frozenset(single_ids))):
            return orc.transformer_forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids,
                                           guidance=guidance, controlnet_block_samples=controlnet_block_samples)
    return forward


def loop_slot(B, T, double_ids, single_ids):
    """denoise_loop_reference(image_prompt=): the forward above at a guided step (2B rows), the oracle's own forward at an unguided one
    (B rows: the positive half alone, no mask in any block)."""
    perturbed = forward_under(T, double_ids, single_ids)

    def forward(p, cfg, hidden_states, *args, ip_params=None, ip_scales=None, ip_embeds=None, **kw):
        if hidden_states.shape[0] == B:
            return orc.transformer_forward(p, cfg, hidden_states, *args, **kw)
        assert hidden_states.shape[0] == 2 * B
        return perturbed(p, cfg, hidden_states, *args, **kw)
    z = torch.zeros(B, 1)
    return dict(forward=forward, ip_params=None, ip_scales=None, embeds=z, neg_embeds=z)


def negative_slot(prompt_embeds, pooled, pag_scale):
    """denoise_loop_reference(negative=) of a PAG call: the first half is the positive conditioning, s = 1 + pag_scale (in double)."""
    return dict(prompt_embeds=prompt_embeds, pooled=pooled, scale=1.0 + float(pag_scale))
