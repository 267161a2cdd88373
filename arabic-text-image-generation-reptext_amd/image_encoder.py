"""The vision encoders on the HIP kernels: the image encoders behind ``pipe(..., ip_adapter_image=img)`` — CLIP ViT-L/14 for the
XLabs / diffusers IP-Adapter, SigLIP-so400m for the InstantX one (``image_encoder_class`` picks between them from a directory's
``config.json``). Both are pre-LN ViT towers on the stack CLIP text also runs (``encoder_common._PreLNStack``: the plans and the layer
loop) and share ``_VisionTower``: the patch weight and the input checks; a class keeps its constructor, its state-dict layout, and
what comes before and after the layers.

``CLIPVisionModelWithProjection`` has the class name, constructor config keys, module names and state-dict keys of `transformers`'
class (``vision_model.pre_layrnorm`` in transformers' spelling, ``vision_model.post_layernorm``, a top-level
``visual_projection.weight``), so a local snapshot's ``config.json`` + safetensors load unchanged. The arithmetic is that of
openai/clip-vit-large-patch14: a stride-p patch convolution, a class token, learned positions, ``pre_layrnorm``, pre-LN blocks with
quick_gelu and no mask, ``post_layernorm`` on the class token and the bias-free ``visual_projection``. As for the text encoders,
`transformers` is importable where the tests run, so parity is pinned against the real class (tests/test_image_encoder_gpu.py).

It runs once per image prompt, outside the denoising loop. The patch convolution is rt_patchify_nchw (im2col) + rt_gemm_bf16, whose
epilogue also adds the position embeddings; the residual stream is fp32, as in text_encoders.CLIPTextModel, and starts from the
bf16 output of ``pre_layrnorm``; attention is ONE rt_attention_hd64 launch per layer (csrc/attention_small_head.hip) on the fused
q|k|v buffer with the tokens as they are: S = 257 needs no padding to 64. ``SiglipVisionModel`` is described at its class.

``clip_preprocess`` / ``siglip_preprocess`` are the host side (PIL), the way tokenisation is for the text encoders: the default
steps of CLIPImageProcessor and SiglipImageProcessor.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .config import Config
from .encoder_common import BF16, F32, _H, _W, _WB, _encoder_layers, _mlp_padded, _PreLNStack, _quick_gelu, pad_mlp_to_64  # noqa: F401

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _rgb_images(image, who: str) -> list:
    """``image`` — a PIL image, a uint8 HWC (or HW) numpy array, or a list of them — as a list of RGB PIL images."""
    from PIL import Image

    images = list(image) if isinstance(image, (list, tuple)) else [image]
    if not images:
        raise ValueError(f"{who}: no image")
    out = []
    for im in images:
        if isinstance(im, np.ndarray):
            if im.dtype != np.uint8 or im.ndim not in (2, 3):
                raise TypeError(f"{who}: numpy images must be uint8 [H,W,C] (or [H,W])")
            im = Image.fromarray(im)
        if not isinstance(im, Image.Image):
            raise TypeError(f"{who}: expected a PIL image or a uint8 numpy array, got {type(im)}")
        out.append(im.convert("RGB"))
    return out


def clip_preprocess(image, size: int = 224) -> torch.Tensor:
    """CLIPImageProcessor's defaults on the host: RGB, shortest edge resized to ``size`` (bicubic; the long edge becomes
    int(size·long/short)), centre crop to size², ·1/255, (x − mean)/std with the OpenAI CLIP constants. ``image``: a PIL image, a
    uint8 HWC (or HW) numpy array, or a list of them -> f32 [B,3,size,size]. Within 2 fp32 ulps of transformers' PIL backend
    (expression order), not bit-equal."""
    from PIL import Image

    mean, std = np.asarray(OPENAI_CLIP_MEAN, dtype=np.float32), np.asarray(OPENAI_CLIP_STD, dtype=np.float32)
    out = []
    for im in _rgb_images(image, "clip_preprocess"):
        w, h = im.size
        short, long_ = (w, h) if w <= h else (h, w)
        new_long = int(size * long_ / short)
        nw, nh = (size, new_long) if w <= h else (new_long, size)
        im = im.resize((nw, nh), resample=Image.BICUBIC)
        left, top = (nw - size) // 2, (nh - size) // 2
        im = im.crop((left, top, left + size, top + size))
        x = np.asarray(im, dtype=np.uint8).astype(np.float32) * np.float32(1.0 / 255.0)
        out.append(((x - mean) / std).transpose(2, 0, 1))
    return torch.from_numpy(np.ascontiguousarray(np.stack(out), dtype=np.float32))


def siglip_preprocess(image, size: int = 384) -> torch.Tensor:
    """SiglipImageProcessor's defaults on the host: RGB, resized straight to size x size (bicubic; no aspect keeping, no crop),
    ·1/255, (x − 0.5)/0.5. ``image``: a PIL image, a uint8 HWC (or HW) numpy array, or a list of them -> f32 [B,3,size,size]."""
    from PIL import Image

    out = []
    for im in _rgb_images(image, "siglip_preprocess"):
        im = im.resize((size, size), resample=Image.BICUBIC)
        x = np.asarray(im, dtype=np.uint8).astype(np.float32) * np.float32(1.0 / 255.0)
        out.append(((x - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1))
    return torch.from_numpy(np.ascontiguousarray(np.stack(out), dtype=np.float32))


def image_encoder_class(directory: str):
    """The encoder class for a model directory, from its ``config.json``: ``model_type`` ``siglip_vision_model``, or ``siglip`` with
    a ``vision_config``, -> SiglipVisionModel; anything else -> CLIPVisionModelWithProjection."""
    with open(os.path.join(directory, "config.json")) as f:
        cfg = json.load(f)
    mt = cfg.get("model_type")
    if mt == "siglip_vision_model" or (mt == "siglip" and isinstance(cfg.get("vision_config"), dict)):
        return SiglipVisionModel
    return CLIPVisionModelWithProjection


class _VisionTower(_PreLNStack):
    """What the two vision encoders add to the shared stack: the patch weight as a GEMM operand, the input checks and
    ``random_init_``. A class names the parameters ``random_init_`` gives unit scale (``_unit_scale``)."""

    _config_section = "vision_config"
    _unit_scale: tuple

    def random_init_(self, seed: int = 0):
        """Random weights at an exercised scale, for tools and tests that run without a checkpoint: matrices at 1/sqrt(fan-in),
        the class token or probe and the positions at unit scale, LayerNorms at identity, biases zero."""
        g = torch.Generator().manual_seed(seed)
        for n, p in self.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.data.fill_(1.0)
            elif n.endswith("bias"):
                p.data.zero_()
            else:
                std = 1.0 if any(u in n for u in self._unit_scale) else p[0].numel() ** -0.5
                p.data.copy_(torch.randn(p.shape, generator=g) * std)
        self._reset_plans()
        return self

    def _tower_plans(self, emb, layers) -> dict:
        """``_layer_plans`` and the patch weight as a GEMM operand [d,Kp]; ``patch_embedding.weight`` becomes a view of its first 3p²
        columns."""
        c = self.config
        d, p, k = c.hidden_size, c.patch_size, 3 * c.patch_size ** 2
        Kp = (k + 63) // 64 * 64                                                  # the GEMM's K % 64 rule: 588 -> 640 for p = 14
        w_patch = torch.zeros(d, Kp, device=self.device, dtype=BF16)
        w_patch[:, :k] = emb.patch_embedding.weight.data.reshape(d, k)
        emb.patch_embedding.weight.data = w_patch[:, :k].view(d, 3, p, p)
        return dict(self._layer_plans(layers), w_patch=w_patch, Kp=Kp)

    def _pixels(self, pixel_values: torch.Tensor) -> torch.Tensor:
        c = self.config
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, c.image_size, c.image_size):
            raise ValueError(f"pixel_values must be [B,3,{c.image_size},{c.image_size}], got {tuple(pixel_values.shape)}")
        if pixel_values.dtype not in (BF16, F32):
            pixel_values = pixel_values.to(F32)
        return pixel_values.to(self.device)


# ========================================================================================================================= CLIP
class CLIPVisionModelOutput(tuple):
    """(image_embeds, last_hidden_state) with attribute access, transformers' field order."""

    def __new__(cls, image_embeds, last_hidden_state):
        obj = super().__new__(cls, (image_embeds, last_hidden_state))
        obj.image_embeds, obj.last_hidden_state = image_embeds, last_hidden_state
        return obj


class CLIPVisionModelWithProjection(_VisionTower):
    _anchor = "visual_projection.weight"
    _unit_scale = ("class_embedding", "position_embedding")
    _head_dim = 64

    def __init__(self, hidden_size: int = 1024, intermediate_size: int = 4096, projection_dim: int = 768, num_hidden_layers: int = 24,
                 num_attention_heads: int = 16, num_channels: int = 3, image_size: int = 224, patch_size: int = 14,
                 hidden_act: str = "quick_gelu", layer_norm_eps: float = 1e-5, device=None, dtype=None, **unused):
        super().__init__()
        if hidden_size % num_attention_heads or hidden_size // num_attention_heads != 64:
            raise ValueError("CLIPVisionModelWithProjection (HIP): head dim must be 64 (ViT-L/14: 1024 / 16; ViT-H's 80 is not built)")
        if hidden_act != "quick_gelu":
            raise ValueError("CLIPVisionModelWithProjection (HIP): only quick_gelu (openai/clip-vit-large-patch14) is implemented")
        if image_size % patch_size:
            raise ValueError(f"CLIPVisionModelWithProjection (HIP): image_size {image_size} is not a multiple of patch_size {patch_size}")
        if num_channels != 3 or projection_dim % 4 or intermediate_size % 64:
            raise ValueError("CLIPVisionModelWithProjection (HIP): 3 channels, projection_dim % 4 == 0 and intermediate_size % 64 == 0")
        self.config = Config(hidden_size=hidden_size, intermediate_size=intermediate_size, projection_dim=projection_dim,
                             num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads, num_channels=num_channels,
                             image_size=image_size, patch_size=patch_size, hidden_act=hidden_act, layer_norm_eps=layer_norm_eps)
        kw = dict(device=device, dtype=dtype)
        vm = _H()
        emb = _H()
        emb.class_embedding = nn.Parameter(torch.empty(hidden_size, **kw), requires_grad=False)
        emb.patch_embedding = _W(hidden_size, num_channels, patch_size, patch_size, **kw)
        emb.position_embedding = _W((image_size // patch_size) ** 2 + 1, hidden_size, **kw)
        vm.embeddings = emb
        vm.pre_layrnorm = _WB(hidden_size, **kw)
        vm.encoder = _encoder_layers(num_hidden_layers, hidden_size, intermediate_size, kw)
        vm.post_layernorm = _WB(hidden_size, **kw)
        self.vision_model = vm
        self.visual_projection = _W(projection_dim, hidden_size, **kw)

    def load_state_dict(self, sd, strict: bool = True, **kw):
        # accept the encoder's keys with or without the `vision_model.` prefix (CLIPVisionModel's own layout), as CLIPTextModel does
        if not any(k.startswith("vision_model.") for k in sd):
            sd = {k if k.startswith("visual_projection.") else "vision_model." + k: v for k, v in sd.items()}
        return self._load(sd, strict, **kw)

    def _build_plans(self):
        return self._tower_plans(self.vision_model.embeddings, self.vision_model.encoder.layers)

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor, output_attentions=None, output_hidden_states=None, interpolate_pos_encoding: bool = False,
                return_dict: bool = True, **unused):
        if output_attentions or output_hidden_states or interpolate_pos_encoding:
            raise NotImplementedError("CLIPVisionModelWithProjection (HIP): only image_embeds and last_hidden_state are produced, at the "
                                      "configured image size")
        plans = self._ensure_plans()
        pixel_values = self._pixels(pixel_values)
        c, dev, vm = self.config, self.device, self.vision_model
        B, d, p = pixel_values.shape[0], c.hidden_size, c.patch_size
        G = c.image_size // p
        S = G * G + 1
        Sp = self._padded_tokens(S)
        eps, aff = float(c.layer_norm_eps), plans["norms"].refresh()
        pre, post = aff[vm.pre_layrnorm], aff[vm.post_layernorm]
        # 1-2. patches -> fp32 rows 1.. of every batch entry, position embeddings added by the GEMM's residual slot; row 0 is the class
        #      token plus its position
        patches = ops.patchify_nchw(pixel_values, p, plans["Kp"])
        pos = vm.embeddings.position_embedding.weight.data.to(F32)
        e = torch.zeros(B, Sp, d, device=dev, dtype=F32) if Sp != S else torch.empty(B, S, d, device=dev, dtype=F32)
        e[:, 0] = pos[0] + vm.embeddings.class_embedding.data
        ops.linear(patches, plans["w_patch"], e[:, 1:S], res=pos[1:].unsqueeze(0).expand(B, -1, -1))
        # 3. pre_layrnorm; its bf16 output starts the fp32 residual stream
        xn = torch.empty(B, Sp, d, device=dev, dtype=BF16)
        ops.layernorm_modulate(e.view(1, B * Sp, d), xn.view(1, B * Sp, d), pre[1], pre[0], eps=eps)
        x = ops.to_f32(xn)
        # 4. the layers, quick_gelu as its own pass over the fc1 output
        self._layers(plans, aff, x, S, act=_quick_gelu)
        last = ops.to_bf16(x)[:, :S]
        # 5-6. post_layernorm on the class token, visual_projection
        pooled = torch.empty(B, 1, d, device=dev, dtype=BF16)
        ops.layernorm_modulate(x[:, 0:1], pooled, post[1].expand(B, -1), post[0].expand(B, -1), eps=eps)
        embeds = torch.empty(B, c.projection_dim, device=dev, dtype=BF16)
        ops.linear(pooled.view(B, d), self.visual_projection.weight.data, embeds)
        return CLIPVisionModelOutput(embeds, last) if return_dict else (embeds, last)

    __call__ = forward


# ======================================================================================================================= SigLIP
class SiglipVisionModelOutput(tuple):
    """(last_hidden_state, pooler_output) with attribute access, transformers' field order."""

    def __new__(cls, last_hidden_state, pooler_output):
        obj = super().__new__(cls, (last_hidden_state, pooler_output))
        obj.last_hidden_state, obj.pooler_output = last_hidden_state, pooler_output
        return obj


class _MHA(nn.Module):
    """torch.nn.MultiheadAttention's parameters (in_proj_weight / in_proj_bias as q|k|v, out_proj)."""

    def __init__(self, d, device=None, dtype=None):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d, d, device=device, dtype=dtype), requires_grad=False)
        self.in_proj_bias = nn.Parameter(torch.empty(3 * d, device=device, dtype=dtype), requires_grad=False)
        self.out_proj = _WB(d, d, device=device, dtype=dtype)


class SiglipVisionModel(_VisionTower):
    """google/siglip-so400m-patch14-384's vision tower with its attention-pooling head: the class name, constructor config keys,
    module names and state-dict keys of `transformers`' class (5.x layout: ``embeddings.*``, ``encoder.layers.*``,
    ``post_layernorm.*``, ``head.*``; a ``vision_model.`` prefix, as in the published checkpoint, is accepted). Arithmetic: patch
    convolution WITH bias + learned positions (no class token, no pre-norm; the convolution keeps image_size // patch_size patches per
    side and drops the rest of the image), pre-LN blocks with gelu_pytorch_tanh, ``post_layernorm`` on all tokens, then the head:
    MHA(probe, h, h), x + mlp(layernorm(x)), row 0. Heads of 72: one rt_attention_hd72 launch per layer on the fused q|k|v buffer
    and one more for the head, whose query is the one row probe·Wqᵀ + bq."""

    _anchor = "head.probe"
    _unit_scale = ("probe", "position_embedding")
    _head_dim = 72

    def __init__(self, hidden_size: int = 1152, intermediate_size: int = 4304, num_hidden_layers: int = 27, num_attention_heads: int = 16,
                 num_channels: int = 3, image_size: int = 384, patch_size: int = 14, hidden_act: str = "gelu_pytorch_tanh",
                 layer_norm_eps: float = 1e-6, vision_use_head: bool = True, device=None, dtype=None, **unused):
        super().__init__()
        if hidden_size % num_attention_heads or hidden_size // num_attention_heads != 72:
            raise ValueError(f"SiglipVisionModel (HIP): head dim must be 72 (so400m: 1152 / 16), got hidden_size {hidden_size} / "
                             f"num_attention_heads {num_attention_heads}")
        if hidden_size % 64:
            raise ValueError(f"SiglipVisionModel (HIP): hidden_size {hidden_size} is not a multiple of 64")
        if hidden_act != "gelu_pytorch_tanh":
            raise ValueError(f"SiglipVisionModel (HIP): only gelu_pytorch_tanh is implemented, got hidden_act '{hidden_act}'")
        if not vision_use_head:
            raise ValueError("SiglipVisionModel (HIP): vision_use_head=False is not supported: pooler_output is what the encoder is for")
        if num_channels != 3 or intermediate_size % 4 or image_size < patch_size:
            raise ValueError("SiglipVisionModel (HIP): 3 channels, intermediate_size % 4 == 0 and image_size >= patch_size")
        self.config = Config(model_type="siglip_vision_model", hidden_size=hidden_size, intermediate_size=intermediate_size,
                             num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads, num_channels=num_channels,
                             image_size=image_size, patch_size=patch_size, hidden_act=hidden_act, layer_norm_eps=layer_norm_eps)
        kw = dict(device=device, dtype=dtype)
        emb = _H()
        emb.patch_embedding = _H()                                               # Conv2d(3, d, kernel p, stride p) WITH bias
        emb.patch_embedding.weight = nn.Parameter(torch.empty(hidden_size, num_channels, patch_size, patch_size, **kw), requires_grad=False)
        emb.patch_embedding.bias = nn.Parameter(torch.empty(hidden_size, **kw), requires_grad=False)
        emb.position_embedding = _W((image_size // patch_size) ** 2, hidden_size, **kw)
        self.embeddings = emb
        self.encoder = _encoder_layers(num_hidden_layers, hidden_size, intermediate_size, kw)
        self.post_layernorm = _WB(hidden_size, **kw)
        head = _H()
        head.probe = nn.Parameter(torch.empty(1, 1, hidden_size, **kw), requires_grad=False)
        head.attention = _MHA(hidden_size, **kw)
        head.layernorm = _WB(hidden_size, **kw)
        head.mlp = _H()
        head.mlp.fc1, head.mlp.fc2 = _WB(intermediate_size, hidden_size, **kw), _WB(hidden_size, intermediate_size, **kw)
        self.head = head

    def load_state_dict(self, sd, strict: bool = True, **kw):
        # a full SiglipModel checkpoint: the text tower and the two logit scalars are not ours; then the published prefix
        sd = {k: v for k, v in sd.items() if not (k.startswith("text_model.") or k in ("logit_scale", "logit_bias"))}
        sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}
        return self._load(sd, strict, **kw)

    def _build_plans(self):
        emb, att, d = self.embeddings, self.head.attention, self.config.hidden_size
        return dict(self._tower_plans(emb, self.encoder.layers), b_patch=emb.patch_embedding.bias.data, wq=att.in_proj_weight.data[:d],
                    bq=att.in_proj_bias.data[:d], wkv=att.in_proj_weight.data[d:], bkv=att.in_proj_bias.data[d:], wo=att.out_proj.weight.data,
                    bo=att.out_proj.bias.data, head_mlp=_mlp_padded(self.head.mlp))

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor, output_attentions=None, output_hidden_states=None, interpolate_pos_encoding: bool = False,
                return_dict: bool = True, **unused):
        if output_attentions or output_hidden_states or interpolate_pos_encoding:
            raise NotImplementedError("SiglipVisionModel (HIP): only last_hidden_state and pooler_output are produced, at the configured "
                                      "image size")
        plans = self._ensure_plans()
        pixel_values = self._pixels(pixel_values)
        c, dev = self.config, self.device
        B, d, H, p = pixel_values.shape[0], c.hidden_size, c.num_attention_heads, c.patch_size
        G = c.image_size // p
        S = G * G
        eps, scale, aff = float(c.layer_norm_eps), 72 ** -0.5, plans["norms"].refresh()
        post, head_ln = aff[self.post_layernorm], aff[self.head.layernorm]
        # 1. patches of the top-left G·p square (384 -> 378 for p = 14: the convolution drops the rest; patchify_nchw copies the crop
        #    once) -> the fp32 residual stream: bias in the GEMM's bias slot, the position table in its residual slot
        patches = ops.patchify_nchw(pixel_values[:, :, : G * p, : G * p], p, plans["Kp"])
        x = torch.empty(B, S, d, device=dev, dtype=F32)
        ops.linear(patches, plans["w_patch"], x, bias=plans["b_patch"], res=self.embeddings.position_embedding.weight.data.to(F32).unsqueeze(0).expand(B, -1, -1))
        # 2. the layers, gelu_tanh in fc1's epilogue
        self._layers(plans, aff, x, S)
        # 3. post_layernorm on all tokens
        last = torch.empty(B, S, d, device=dev, dtype=BF16)
        ops.layernorm_modulate(x.view(1, B * S, d), last.view(1, B * S, d), post[1], post[0], eps=eps)
        # 4. the attention-pooling head: k|v of the normed tokens in one GEMM, one probe row per batch entry, out_proj, MLP
        kv = torch.empty(B, S, 2 * d, device=dev, dtype=BF16)
        ops.linear(last.view(B * S, d), plans["wkv"], kv.view(B * S, 2 * d), bias=plans["bkv"])
        pa = torch.empty(B, 1, d, device=dev, dtype=BF16)
        q_probe = (self.head.probe.data.to(F32).reshape(1, d) @ plans["wq"].to(F32).t() + plans["bq"]).to(BF16).reshape(1, 1, d)
        ops.attention_hd72(q_probe, kv[..., :d], kv[..., d:], pa, H, scale)
        y = torch.empty(B, d, device=dev, dtype=F32)
        ops.linear(pa.view(B, d), plans["wo"], y, bias=plans["bo"])
        yn = torch.empty(1, B, d, device=dev, dtype=BF16)
        ops.layernorm_modulate(y.view(1, B, d), yn, head_ln[1], head_ln[0], eps=eps)
        hw1, hb1, hw2, hb2 = plans["head_mlp"]
        hh = torch.empty(B, hw1.shape[0], device=dev, dtype=BF16)
        ops.linear(yn.view(B, d), hw1, hh, bias=hb1, gelu_from=0)
        ops.linear(hh, hw2, y, bias=hb2, res=y)
        pooled = ops.to_bf16(y)
        return SiglipVisionModelOutput(last, pooled) if return_dict else (last, pooled)

    __call__ = forward
