"""fp32 CPU restatement of per-line prompts for the tests (a plain helper module, not a conftest).

The transformer reads cat([base prompt, line 1, ..., line R]) as its text stream (text ids zeros) and its joint attention is the oracle's
with -inf on the hidden keys:

    row i attends key j  iff  bit g(j) of row_vis[b][i] is set,    g(j) = the key group that holds j (``visible``)

Everything else is oracle.flux_oracle's own code: ``transformer_forward`` runs ``orc.transformer_forward`` while ``orc.attention`` is
replaced by ``masked_attention``, which keeps that function's rounding points under ``orc.stored_as``: the row sums come from the
unrounded numerators, the numerators are rounded as the second product's operand, the output is rounded once. The towers never see a
line prompt: ``loop_forward`` gives ``loop_reference.denoise_loop_reference`` a transformer forward (its ``image_prompt["forward"]``
slot) that appends the line embeddings and picks the rows of the table that belong to the batch it is called with ([negative, positive]
at 2B, the positive half at B)."""
import contextlib
import math

import numpy as np
import torch

from oracle import flux_oracle as orc


def visible(ends, row_vis):
    """bool [B, S, S] from the key-group ends and the int32 row table [B, S]: the contract restated, not imported."""
    S = int(ends[-1])
    group = np.searchsorted(np.asarray(ends), np.arange(S), side="right").astype(np.uint32)
    words = row_vis.cpu().numpy().view(np.uint32)
    return torch.from_numpy(((words[:, :, None] >> group[None, None, :]) & 1).astype(bool))


def masked_attention(see):
    """orc.attention with the scores of hidden keys at -inf; see: bool [B or 1, S, S]. Every row must see a key."""
    def attention(q, k, v):
        B, S, H, Dh = q.shape
        qh, kh, vh = (t.permute(0, 2, 1, 3) for t in (q, k, v))
        s = (qh @ kh.transpose(-1, -2)) / math.sqrt(Dh)
        s = s.masked_fill(~see[:, None].expand(B, H, S, S), float("-inf"))
        if orc._STORE is None:
            o = torch.softmax(s, dim=-1) @ vh
        else:
            e = torch.exp(s - s.amax(dim=-1, keepdim=True))
            o = (orc._s(e) @ vh) / e.sum(dim=-1, keepdim=True)
        return orc._s(o.permute(0, 2, 1, 3).reshape(B, S, H * Dh))
    return attention


@contextlib.contextmanager
def attention_as(fn):
    saved = orc.attention
    orc.attention = fn
    try:
        yield
    finally:
        orc.attention = saved


def transformer_forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                        controlnet_block_samples=None, line_embeds=None, ends=None, row_vis=None):
    """orc.transformer_forward on cat([encoder_hidden_states, line_embeds]) under the mask of (ends, row_vis [B, S])."""
    pe = torch.cat([encoder_hidden_states, line_embeds], dim=1)
    with attention_as(masked_attention(visible(ends, row_vis))):
        return orc.transformer_forward(p, cfg, hidden_states, pe, pooled_projections, timestep, img_ids, torch.zeros(pe.shape[1], 3),
                                       guidance=guidance, controlnet_block_samples=controlnet_block_samples)


def loop_forward(line_embeds, ends, row_vis):
    """The ``forward`` of denoise_loop_reference's image_prompt slot for a call with line prompts. line_embeds [B, R·L, D] of the positive
    half (both halves read the same); row_vis [B, S], or [2B, S] under true CFG ([negative, positive])."""
    def forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                controlnet_block_samples=None, **unused):
        Bc = hidden_states.shape[0]
        le = line_embeds if Bc == line_embeds.shape[0] else torch.cat([line_embeds, line_embeds], dim=0)
        return transformer_forward(p, cfg, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=guidance,
                                   controlnet_block_samples=controlnet_block_samples, line_embeds=le, ends=ends, row_vis=row_vis[-Bc:])
    return forward


def image_prompt_slot(line_embeds, ends, row_vis):
    """What denoise_loop_reference(image_prompt=) takes: the forward above and inert values for the adapter's own entries."""
    z = torch.zeros(line_embeds.shape[0], 1)
    return dict(forward=loop_forward(line_embeds, ends, row_vis), ip_params=None, ip_scales=None, embeds=z, neg_embeds=z)
