"""CLIP vision encoder on the HIP kernels: the image encoder behind ``pipe(..., ip_adapter_image=img)``.

``CLIPVisionModelWithProjection`` has the class name, constructor config keys, module names and state-dict keys of `transformers`'
class (``vision_model.pre_layrnorm`` in transformers' spelling, ``vision_model.post_layernorm``, a top-level
``visual_projection.weight``), so a local snapshot's ``config.json`` + safetensors load unchanged. The arithmetic is that of
openai/clip-vit-large-patch14: a stride-p patch convolution, a class token, learned positions, ``pre_layrnorm``, pre-LN blocks with
quick_gelu and no mask, ``post_layernorm`` on the class token and the bias-free ``visual_projection``. As for the text encoders,
`transformers` is importable where the tests run, so parity is pinned against the real class (tests/test_image_encoder_gpu.py).

It runs once per image prompt, outside the denoising loop. The patch convolution is rt_patchify_nchw (im2col) + rt_gemm_bf16, whose
epilogue also adds the position embeddings; the residual stream is fp32, as in text_encoders.CLIPTextModel, and starts from the
bf16 output of ``pre_layrnorm``; attention is ONE rt_attention_hd64 launch per layer (csrc/attention_hd64.hip) on the fused q|k|v
buffer with the tokens as they are: S = 257 needs no padding to 64.

``clip_preprocess`` is the host side (PIL), the way tokenisation is for the text encoders: CLIPImageProcessor's default steps.
"""
from __future__ import annotations

import json
import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import native, ops
from .config import Config
from .modules import WeightsIO
from .text_encoders import BF16, F32, _H, _W, _WB, _stream

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_preprocess(image, size: int = 224) -> torch.Tensor:
    """CLIPImageProcessor's defaults on the host: RGB, shortest edge resized to ``size`` (bicubic; the long edge becomes
    int(size·long/short)), centre crop to size², ·1/255, (x − mean)/std with the OpenAI CLIP constants. ``image``: a PIL image, a
    uint8 HWC (or HW) numpy array, or a list of them -> f32 [B,3,size,size]. Within 2 fp32 ulps of transformers' PIL backend
    (expression order), not bit-equal."""
    from PIL import Image

    images = list(image) if isinstance(image, (list, tuple)) else [image]
    if not images:
        raise ValueError("clip_preprocess: no image")
    mean, std = np.asarray(OPENAI_CLIP_MEAN, dtype=np.float32), np.asarray(OPENAI_CLIP_STD, dtype=np.float32)
    out = []
    for im in images:
        if isinstance(im, np.ndarray):
            if im.dtype != np.uint8 or im.ndim not in (2, 3):
                raise TypeError("clip_preprocess: numpy images must be uint8 [H,W,C] (or [H,W])")
            im = Image.fromarray(im)
        if not isinstance(im, Image.Image):
            raise TypeError(f"clip_preprocess: expected a PIL image or a uint8 numpy array, got {type(im)}")
        im = im.convert("RGB")
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


class CLIPVisionModelOutput(tuple):
    """(image_embeds, last_hidden_state) with attribute access, transformers' field order."""

    def __new__(cls, image_embeds, last_hidden_state):
        obj = super().__new__(cls, (image_embeds, last_hidden_state))
        obj.image_embeds, obj.last_hidden_state = image_embeds, last_hidden_state
        return obj


class CLIPVisionModelWithProjection(nn.Module, WeightsIO):
    config_name = "config.json"
    weights_name = "model.safetensors"

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
        enc = _H()
        enc.layers = nn.ModuleList()
        for _ in range(num_hidden_layers):
            l = _H()
            sa = _H()
            sa.q_proj, sa.k_proj, sa.v_proj, sa.out_proj = (_WB(hidden_size, hidden_size, **kw) for _ in range(4))
            l.self_attn = sa
            l.layer_norm1, l.layer_norm2 = _WB(hidden_size, **kw), _WB(hidden_size, **kw)
            mlp = _H()
            mlp.fc1, mlp.fc2 = _WB(intermediate_size, hidden_size, **kw), _WB(hidden_size, intermediate_size, **kw)
            l.mlp = mlp
            enc.layers.append(l)
        vm.encoder = enc
        vm.post_layernorm = _WB(hidden_size, **kw)
        self.vision_model = vm
        self.visual_projection = _W(projection_dim, hidden_size, **kw)
        self._plans = None

    @property
    def dtype(self):
        return self.visual_projection.weight.dtype

    @property
    def device(self):
        return self.visual_projection.weight.device

    def _apply(self, fn, *a, **k):
        self._plans = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, sd, strict: bool = True, **kw):
        # accept the encoder's keys with or without the `vision_model.` prefix (CLIPVisionModel's own layout), as CLIPTextModel does
        if not any(k.startswith("vision_model.") for k in sd):
            sd = {k if k.startswith("visual_projection.") else "vision_model." + k: v for k, v in sd.items()}
        sd = {k: v for k, v in sd.items() if not k.endswith("position_ids")}
        self._plans = None
        return super().load_state_dict(sd, strict=strict, **kw)

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=None, subfolder: Optional[str] = None, device=None, **unused):
        d = cls._resolve_dir(path, subfolder)
        with open(os.path.join(d, cls.config_name)) as f:
            cfg = json.load(f)
        cfg = cfg.get("vision_config", cfg)
        m = cls(**cfg, device=device or "cpu", dtype=torch_dtype or BF16)
        m.load_state_dict({k: v.to(torch_dtype or BF16) for k, v in cls._load_safetensors_dir(d).items()}, strict=True)
        return m

    def random_init_(self, seed: int = 0):
        """Random weights at an exercised scale, for tools and tests that run without a checkpoint: matrices at 1/sqrt(fan-in),
        embeddings at unit scale, LayerNorms at identity, biases zero."""
        g = torch.Generator().manual_seed(seed)
        for n, p in self.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.data.fill_(1.0)
            elif n.endswith("bias"):
                p.data.zero_()
            else:
                std = 1.0 if p.dim() == 1 or "position_embedding" in n else p[0].numel() ** -0.5
                p.data.copy_(torch.randn(p.shape, generator=g) * std)
        self._plans = None
        return self

    def _ensure_plans(self):
        if self._plans is not None:
            return self._plans
        if self.dtype != BF16 or not self.visual_projection.weight.is_cuda:
            raise RuntimeError("CLIPVisionModelWithProjection (HIP): bf16 on the GPU only; there is no CPU fallback")

        def affine(ln):           # LayerNorm(x)·w + b == LN(x)·(1 + (w - 1)) + b: the adaLN kernel with constant vectors
            return (ln.weight.data.to(F32) - 1.0).reshape(1, -1).contiguous(), ln.bias.data.to(F32).reshape(1, -1).contiguous()

        c, vm = self.config, self.vision_model
        d, k = c.hidden_size, 3 * c.patch_size ** 2
        Kp = (k + 63) // 64 * 64                                                  # the GEMM's K % 64 rule: 588 -> 640 for p = 14
        w_patch = torch.zeros(d, Kp, device=self.device, dtype=BF16)
        w_patch[:, :k] = vm.embeddings.patch_embedding.weight.data.reshape(d, k)
        pos = vm.embeddings.position_embedding.weight.data.to(F32)
        cls_row = (vm.embeddings.class_embedding.data.to(F32) + pos[0]).contiguous()   # the class row is a constant of the weights
        layers = []
        for l in vm.encoder.layers:
            sa = l.self_attn
            wqkv = torch.cat([sa.q_proj.weight.data, sa.k_proj.weight.data, sa.v_proj.weight.data], dim=0).contiguous()
            bqkv = torch.cat([sa.q_proj.bias.data, sa.k_proj.bias.data, sa.v_proj.bias.data], dim=0).contiguous()
            layers.append((wqkv, bqkv, sa.out_proj.weight.data, sa.out_proj.bias.data, l.mlp.fc1.weight.data, l.mlp.fc1.bias.data,
                           l.mlp.fc2.weight.data, l.mlp.fc2.bias.data, affine(l.layer_norm1), affine(l.layer_norm2)))
        self._plans = dict(w_patch=w_patch, Kp=Kp, pos_patches=pos[1:].contiguous(), cls_row=cls_row, pre=affine(vm.pre_layrnorm),
                           post=affine(vm.post_layernorm), layers=layers)
        return self._plans

    # The two hooks tools/bench_image_encoder.py overrides to time the per-head assembled attention on the same forward.
    def _padded_tokens(self, S: int) -> int:
        """Rows per batch entry of the token buffers: the fused attention takes S as it is."""
        return S

    def _attention(self, qkv: torch.Tensor, att: torch.Tensor, S: int) -> None:
        d, H = self.config.hidden_size, self.config.num_attention_heads
        ops.attention_hd64(qkv[:, :S, :d], qkv[:, :S, d : 2 * d], qkv[:, :S, 2 * d :], att[:, :S], H, 64 ** -0.5)

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor, output_attentions=None, output_hidden_states=None, interpolate_pos_encoding: bool = False,
                return_dict: bool = True, **unused):
        if output_attentions or output_hidden_states or interpolate_pos_encoding:
            raise NotImplementedError("CLIPVisionModelWithProjection (HIP): only image_embeds and last_hidden_state are produced, at the "
                                      "configured image size")
        plans = self._ensure_plans()
        c, dev, lib = self.config, self.device, native.load()
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, c.image_size, c.image_size):
            raise ValueError(f"pixel_values must be [B,3,{c.image_size},{c.image_size}], got {tuple(pixel_values.shape)}")
        if pixel_values.dtype not in (BF16, F32):
            pixel_values = pixel_values.to(F32)
        pixel_values = pixel_values.to(dev)
        B, d, F_, p = pixel_values.shape[0], c.hidden_size, c.intermediate_size, c.patch_size
        G = c.image_size // p
        S = G * G + 1
        Sp = self._padded_tokens(S)
        eps = float(c.layer_norm_eps)
        # 1-2. patches -> fp32 rows 1.. of every batch entry, position embeddings added by the GEMM's residual slot; row 0 is constant
        patches = ops.patchify_nchw(pixel_values, p, plans["Kp"])
        e = torch.zeros(B, Sp, d, device=dev, dtype=F32) if Sp != S else torch.empty(B, S, d, device=dev, dtype=F32)
        e[:, 0] = plans["cls_row"]
        ops.linear(patches, plans["w_patch"], e[:, 1:S], res=plans["pos_patches"].unsqueeze(0).expand(B, -1, -1))
        # 3. pre_layrnorm; its bf16 output starts the fp32 residual stream
        xn = torch.empty(B, Sp, d, device=dev, dtype=BF16)
        e2, xn2 = e.view(1, B * Sp, d), xn.view(1, B * Sp, d)
        ops.layernorm_modulate(e2, xn2, plans["pre"][1], plans["pre"][0], eps=eps)
        x = ops.to_f32(xn)
        x2, x3 = x.view(B * Sp, d), x.view(1, B * Sp, d)
        qkv = torch.empty(B, Sp, 3 * d, device=dev, dtype=BF16)
        att = torch.zeros(B, Sp, d, device=dev, dtype=BF16) if Sp != S else torch.empty(B, S, d, device=dev, dtype=BF16)
        hid = torch.empty(B * Sp, F_, device=dev, dtype=BF16)
        # 4. the layers
        for wqkv, bqkv, wo, bo, w1, b1, w2, b2, ln1, ln2 in plans["layers"]:
            ops.layernorm_modulate(x3, xn2, ln1[1], ln1[0], eps=eps)
            ops.linear(xn.view(B * Sp, d), wqkv, qkv.view(B * Sp, 3 * d), bias=bqkv)
            self._attention(qkv, att, S)
            ops.linear(att.view(B * Sp, d), wo, x2, bias=bo, res=x2)
            ops.layernorm_modulate(x3, xn2, ln2[1], ln2[0], eps=eps)
            ops.linear(xn.view(B * Sp, d), w1, hid, bias=b1)
            native.check("rt_quick_gelu", lib.rt_quick_gelu(hid.data_ptr(), hid.numel(), _stream()))
            ops.linear(hid, w2, x2, bias=b2, res=x2)
        last = ops.to_bf16(x)[:, :S]
        # 5-6. post_layernorm on the class token, visual_projection
        pooled = torch.empty(B, 1, d, device=dev, dtype=BF16)
        ops.layernorm_modulate(x[:, 0:1], pooled, plans["post"][1].expand(B, -1), plans["post"][0].expand(B, -1), eps=eps)
        embeds = torch.empty(B, c.projection_dim, device=dev, dtype=BF16)
        ops.linear(pooled.view(B, d), self.visual_projection.weight.data, embeds)
        return CLIPVisionModelOutput(embeds, last) if return_dict else (embeds, last)

    __call__ = forward
