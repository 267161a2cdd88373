"""Prompt encoders on the HIP kernels: T5-v1.1 encoder (FLUX's text_encoder_2: T5-XXL) and the CLIP text
model (text_encoder: CLIP-L), as `FluxControlNetPipeline` calls them (PIPE:232-347):

    prompt_embeds = text_encoder_2(input_ids, output_hidden_states=False)[0]              # [B, 512, 4096], no attention mask
    pooled        = text_encoder(input_ids, output_hidden_states=False).pooler_output     # [B, 768]

Same class names, constructor config keys and state-dict keys as `transformers`' T5EncoderModel / CLIPTextModel, so a local
snapshot's `config.json` + safetensors load unchanged; the arithmetic follows their published definitions (pre-norm T5 blocks with
T5LayerNorm, un-scaled dot products plus the shared bucketed relative-position bias, gated tanh-GELU feed-forward; pre-LN CLIP
blocks with a causal mask, learned positions, quick_gelu, final LayerNorm, pooled = hidden state at the EOS position).
`transformers` itself is importable in the build container, so — unlike the diffusers-side math — THIS part's parity is pinned:
tests/test_text_encoders_gpu.py compares against the real classes with shared random weights.

They run once per prompt, outside the denoising loop. Matrix work goes through rt_gemm_bf16 (fp32 residual stream); attention has
head dim 64 and a bias/mask, so it is assembled per (batch, head) from GEMM + rt_softmax_rows_bias + rt_transpose_bf16 + GEMM.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import native, ops
from .ops import _dev
from .config import Config
from .encoder_common import (BF16, F32, _H, _W, _WB, _AssembledAttention, _attention_heads, _attention_scratch, _Encoder,  # noqa: F401
                             _encoder_layers, _fuse, _PreLNStack, _quick_gelu, _stream, pad_mlp_to_64)


class BaseModelOutput(tuple):
    """Tuple-like result with attribute access, the two ways the pipeline reads encoder outputs."""

    def __new__(cls, last_hidden_state, pooler_output=None):
        obj = super().__new__(cls, (last_hidden_state,) if pooler_output is None else (last_hidden_state, pooler_output))
        obj.last_hidden_state, obj.pooler_output = last_hidden_state, pooler_output
        return obj


def _ids_i32(input_ids: torch.Tensor, device) -> torch.Tensor:
    return input_ids.to(device=device, dtype=torch.int32).contiguous()


# =========================================================================================================== T5
def t5_relative_position_bucket(rel: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    """Bidirectional bucketing of T5 (Raffel et al. 2020, mesh-tensorflow `_relative_position_bucket`): half the buckets per sign,
    exact up to num_buckets/4, logarithmic up to max_distance."""
    nb = num_buckets // 2
    ret = (rel > 0).to(torch.long) * nb
    n = rel.abs()
    max_exact = nb // 2
    is_small = n < max_exact
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return ret + torch.where(is_small, n, large)


class T5EncoderModel(_Encoder):
    _anchor = "shared.weight"

    def __init__(self, vocab_size: int = 32128, d_model: int = 4096, d_kv: int = 64, d_ff: int = 10240, num_layers: int = 24,
                 num_heads: int = 64, relative_attention_num_buckets: int = 32, relative_attention_max_distance: int = 128,
                 layer_norm_epsilon: float = 1e-6, feed_forward_proj: str = "gated-gelu", device=None, dtype=None, **unused):
        super().__init__()
        if d_kv != 64:
            raise ValueError("T5EncoderModel (HIP): d_kv must be 64 (T5 v1.1 / FLUX's T5-XXL)")
        if feed_forward_proj != "gated-gelu":
            raise ValueError("T5EncoderModel (HIP): only the v1.1 gated-gelu feed-forward is implemented")
        self.config = Config(vocab_size=vocab_size, d_model=d_model, d_kv=d_kv, d_ff=d_ff, num_layers=num_layers, num_heads=num_heads,
                             relative_attention_num_buckets=relative_attention_num_buckets,
                             relative_attention_max_distance=relative_attention_max_distance, layer_norm_epsilon=layer_norm_epsilon,
                             feed_forward_proj=feed_forward_proj)
        kw = dict(device=device, dtype=dtype)
        inner = num_heads * d_kv
        self.shared = _W(vocab_size, d_model, **kw)
        enc = _H()
        enc.block = nn.ModuleList()
        for i in range(num_layers):
            blk = _H()
            l0, l1 = _H(), _H()
            sa = _H()
            sa.q, sa.k, sa.v = _W(inner, d_model, **kw), _W(inner, d_model, **kw), _W(inner, d_model, **kw)
            sa.o = _W(d_model, inner, **kw)
            if i == 0:
                sa.relative_attention_bias = _W(relative_attention_num_buckets, num_heads, **kw)
            l0.SelfAttention, l0.layer_norm = sa, _W(d_model, **kw)
            ff = _H()
            ff.wi_0, ff.wi_1, ff.wo = _W(d_ff, d_model, **kw), _W(d_ff, d_model, **kw), _W(d_model, d_ff, **kw)
            l1.DenseReluDense, l1.layer_norm = ff, _W(d_model, **kw)
            blk.layer = nn.ModuleList([l0, l1])
            enc.block.append(blk)
        enc.final_layer_norm = _W(d_model, **kw)
        self.encoder = enc

    def load_state_dict(self, sd, strict: bool = True, **kw):
        return self._load({k: v for k, v in sd.items() if k != "encoder.embed_tokens.weight"}, strict, **kw)      # tied to `shared`

    def _build_plans(self):
        plans = []
        for blk in self.encoder.block:
            sa, ff = blk.layer[0].SelfAttention, blk.layer[1].DenseReluDense
            qkv, wi = _fuse([sa.q, sa.k, sa.v])[0], _fuse([ff.wi_1, ff.wi_0])[0]                # wi: [linear | gelu] halves
            plans.append((qkv, sa.o.weight.data, wi, ff.wo.weight.data, blk.layer[0].layer_norm.weight.data, blk.layer[1].layer_norm.weight.data))
        self._buckets = {}
        return plans

    def _position_bias(self, T: int) -> torch.Tensor:
        """[H, T, T] f32: relative_attention_bias[bucket(key - query)], shared by all layers (it lives in block 0)."""
        if T not in self._buckets:                                               # a function of T alone: kept; the table is read on every call
            c = self.config
            ctx = torch.arange(T)[:, None]
            mem = torch.arange(T)[None, :]
            buckets = t5_relative_position_bucket(mem - ctx, c.relative_attention_num_buckets, c.relative_attention_max_distance)
            self._buckets = {T: buckets.to(self.device)}
        table = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.data.to(F32)     # [buckets, H]
        return table[self._buckets[T]].permute(2, 0, 1).contiguous()

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask=None, output_hidden_states: bool = False, return_dict: bool = True, **unused):
        if attention_mask is not None:
            raise NotImplementedError("T5EncoderModel (HIP): the FLUX pipelines pass no attention mask (PIPE:287-289)")
        plans = self._ensure_plans()
        c = self.config
        dev = self.device
        B, T = input_ids.shape
        if T % 64:
            raise ValueError("T5EncoderModel (HIP): sequence length must be a multiple of 64 (the pipelines pad to 512)")
        d, H, F_ = c.d_model, c.num_heads, c.d_ff
        inner = H * 64
        ids = _ids_i32(input_ids.reshape(-1), dev)
        emb = torch.empty(B * T, d, device=dev, dtype=BF16)
        native.call("rt_embedding_gather", _dev(self.shared.weight.data, "shared", BF16), d, _dev(ids, "ids", torch.int32), _dev(emb, "emb", BF16), d,
                    B * T, d, c.vocab_size, _stream())
        x = ops.to_f32(emb)                                                     # fp32 residual stream [B*T, d]
        xn = torch.empty(B * T, d, device=dev, dtype=BF16)
        qkv = torch.empty(B, T, 3 * inner, device=dev, dtype=BF16)
        att = torch.empty(B, T, inner, device=dev, dtype=BF16)
        hid = torch.empty(B * T, 2 * F_, device=dev, dtype=BF16)
        act = torch.empty(B * T, F_, device=dev, dtype=BF16)
        scratch = _attention_scratch(T, dev)
        bias = self._position_bias(T)
        eps = float(c.layer_norm_epsilon)

        def rms(w, dst):
            native.call("rt_rmsnorm_rows", _dev(x, "x", F32), d, 1, _dev(w, "w", BF16), _dev(dst, "out", BF16), d, B * T, d, eps, _stream())

        for wqkv, wo, wi, wff, ln0, ln1 in plans:
            rms(ln0, xn)
            ops.linear(xn, wqkv, qkv.view(B * T, 3 * inner))
            _attention_heads(qkv[..., :inner], qkv[..., inner : 2 * inner], qkv[..., 2 * inner :], att, H, bias, 1.0, T, T, scratch)
            ops.linear(att.view(B * T, inner), wo, x, res=x)
            rms(ln1, xn)
            ops.linear(xn, wi, hid, gelu_from=F_)                                # [wi_1 x | gelu(wi_0 x)]
            native.call("rt_gated_mul", _dev(hid, "hid", BF16), 2 * F_, _dev(act, "act", BF16), F_, B * T, F_, _stream())
            ops.linear(act, wff, x, res=x)
        out = torch.empty(B * T, d, device=dev, dtype=BF16)
        rms(self.encoder.final_layer_norm.weight.data, out)
        out = out.view(B, T, d)
        return BaseModelOutput(out) if return_dict else (out,)

    __call__ = forward


# =========================================================================================================== CLIP
class CLIPTextModel(_AssembledAttention, _PreLNStack):
    _anchor = "text_model.final_layer_norm.weight"
    _config_section = "text_config"

    def __init__(self, vocab_size: int = 49408, hidden_size: int = 768, intermediate_size: int = 3072, num_hidden_layers: int = 12,
                 num_attention_heads: int = 12, max_position_embeddings: int = 77, hidden_act: str = "quick_gelu",
                 layer_norm_eps: float = 1e-5, eos_token_id: int = 2, device=None, dtype=None, **unused):
        super().__init__()
        if hidden_size % num_attention_heads or hidden_size // num_attention_heads != 64:
            raise ValueError("CLIPTextModel (HIP): head dim must be 64 (CLIP-L: 768 / 12)")
        if hidden_act != "quick_gelu":
            raise ValueError("CLIPTextModel (HIP): only quick_gelu (openai/clip-vit-large-patch14) is implemented")
        self.config = Config(vocab_size=vocab_size, hidden_size=hidden_size, intermediate_size=intermediate_size,
                             num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                             max_position_embeddings=max_position_embeddings, hidden_act=hidden_act, layer_norm_eps=layer_norm_eps,
                             eos_token_id=eos_token_id)
        kw = dict(device=device, dtype=dtype)
        tm = _H()
        emb = _H()
        emb.token_embedding = _W(vocab_size, hidden_size, **kw)
        emb.position_embedding = _W(max_position_embeddings, hidden_size, **kw)
        tm.embeddings = emb
        tm.encoder = _encoder_layers(num_hidden_layers, hidden_size, intermediate_size, kw)
        tm.final_layer_norm = _WB(hidden_size, **kw)
        self.text_model = tm

    def load_state_dict(self, sd, strict: bool = True, **kw):
        # transformers >= 5 saves the text model's keys without the `text_model.` prefix; accept both layouts
        if not any(k.startswith("text_model.") for k in sd):
            sd = {"text_model." + k: v for k, v in sd.items()}
        return self._load(sd, strict, **kw)

    def _build_plans(self):
        return self._layer_plans(self.text_model.encoder.layers)

    def _attention_bias(self, S, device):
        return torch.full((1, S, S), float("-inf"), device=device, dtype=F32).triu_(1).contiguous()     # causal: -inf above the diagonal

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask=None, output_hidden_states: bool = False, return_dict: bool = True, **unused):
        if attention_mask is not None:
            raise NotImplementedError("CLIPTextModel (HIP): the FLUX pipelines pass no attention mask (PIPE:337-339)")
        plans = self._ensure_plans()
        tm, c, dev = self.text_model, self.config, self.device
        B, T = input_ids.shape
        if T > c.max_position_embeddings:
            raise ValueError("sequence longer than max_position_embeddings")
        Tp = self._padded_tokens(T)
        d = c.hidden_size
        ids = torch.zeros(B, Tp, dtype=torch.int32, device=dev)
        ids[:, :T] = input_ids.to(dev, torch.int32)
        emb = torch.empty(B * Tp, d, device=dev, dtype=BF16)
        native.call("rt_embedding_gather", _dev(tm.embeddings.token_embedding.weight.data, "token_embedding", BF16), d, _dev(ids, "ids", torch.int32),
                    _dev(emb, "emb", BF16), d, B * Tp, d, c.vocab_size, _stream())
        pos = torch.zeros(Tp, d, device=dev, dtype=BF16)
        pos[:T] = tm.embeddings.position_embedding.weight.data[:T]
        x = ops.to_f32(emb).view(B, Tp, d)
        for b in range(B):                                                        # x[b] += position embeddings
            ops.masked_accumulate_(x[b : b + 1], pos.unsqueeze(0), None, 1.0, True)
        aff = plans["norms"].refresh()
        self._layers(plans, aff, x, T, act=_quick_gelu)
        final_ln = aff[tm.final_layer_norm]
        out = torch.empty(B, Tp, d, device=dev, dtype=BF16)
        ops.layernorm_modulate(x.view(1, B * Tp, d), out.view(1, B * Tp, d), final_ln[1], final_ln[0], eps=float(c.layer_norm_eps))
        last = out[:, :T]
        idc = input_ids.to(dev)
        if c.eos_token_id == 2:        # legacy configs: the EOS token has the highest id in the vocabulary
            pos_eos = idc.to(torch.int64).argmax(dim=-1)
        else:
            pos_eos = (idc == c.eos_token_id).to(torch.int64).argmax(dim=-1)
        pooled = last[torch.arange(B, device=dev), pos_eos]
        return BaseModelOutput(last, pooled) if return_dict else (last, pooled)

    __call__ = forward
