"""FLUX IP-Adapter (image prompt): checkpoint reader, adapter state, loop-invariant set-up. Two forms: the diffusers / XLabs one (one
ungated term per double block, below) and the InstantX one (a term inside every block, double and single; further below).

With C = joint_attention_dim, d = inner_dim, H heads of 128, E = image embedding width, n = tokens per image prompt:

  1. tok  = LayerNorm_C(reshape(Linear_{E -> n·C}(embeds), [B, n, C]))      affine, eps 1e-5             once per call
  2. K_i  = to_k_ip_i(tok), V_i = to_v_ip_i(tok)   Linear_{C -> d} + bias, no norm, no RoPE               once per call
  3. ip_i = s_i · softmax(q_i K_iᵀ / √128) V_i     q_i = the block's image query after norm_q, before RoPE  per step (rt_ip_attention)
  4. h   <- h + ip_i  after the block's feed-forward residual (image stream only; no to_out, no gate)

Rules recalled from diffusers (FluxIPAdapterMixin, FluxIPAdapterJointAttnProcessor2_0, ImageProjection, FluxTransformerBlock) and the
XLabs-AI checkpoint layout; parity with them is unpinned (nothing can be checked offline). Single adapter, single image per sample.

The adapter is held on the transformer as ``_ip_adapter`` — plain tensors, NOT registered parameters: ``state_dict()``,
``load_state_dict(strict=True)`` and ``save_pretrained()`` are unchanged; ``_apply`` moves it with the model.

Two key layouts, one table each (``_LAYOUTS``):
  diffusers  image_proj.proj.* / image_proj.norm.* / ip_adapter.{i}.to_k_ip.* / ip_adapter.{i}.to_v_ip.*
  XLabs      ip_adapter_proj_model.proj.* / .norm.* / double_blocks.{i}.processor.ip_adapter_double_stream_k_proj.* / _v_proj.*
Refused with a ValueError naming the key: unknown keys, keys that name single blocks, a block count other than
num_layers, norm width != C, K/V out-features != d or in-features != C, a non-integer or > 128 token count, missing biases.

The InstantX form (``InstantX/FLUX.1-dev-IP-Adapter``; layout "instantx", recognised by ``image_proj.proj.0.weight``), with
L2 = num_layers, L1 = num_single_layers and j over all L2 + L1 blocks, double blocks first:

  1. tok  = LayerNorm_C(reshape(Linear_{2E -> n·C}(GELU(Linear_{E -> 2E}(embeds))), [B, n, C]))   biases, exact (erf) GELU, eps 1e-5
  2. K_j  = rmsnorm_128(to_k_ip_j(tok)), V_j = to_v_ip_j(tok)    Linear_{C -> d} WITHOUT bias; the norm per head, eps 1e-5, no weight,
                                                                  on K only; K rounded to bf16 after the norm; no RoPE
  3. ip_j = softmax(q̂ K_jᵀ / √128) V_j      q̂ = the block's query after norm_q, before RoPE: the image rows of a double block, ALL
                                              S = T + N rows (text rows included) of a single block   (rt_ip_attention_gated)
  4. double block: h <- h + gate_msa · (to_out(attn_img) + s_j · ip_j)     (gated; the text stream is untouched)
     single block: x <- x + gate · proj_out([attn + s_j · ip_j | gelu(mlp)])
  5. s_j: one float per block, default 1.0.

Rules recalled from InstantX's IPAFluxAttnProcessor2_0, MLPProjModel and transformer_flux.py; neither they nor diffusers can be read
offline, so parity with upstream is unpinned here too. What the tests pin is parity with an fp32 restatement of exactly these rules
(tests/instantx_reference.py). Keys: image_proj.proj.{0,2}.{weight,bias}, image_proj.norm.{weight,bias}, ip_adapter.{j}.to_{k,v}_ip.weight
— as a flat dict, a flat .safetensors file, or the upstream ``ip-adapter.bin`` (torch.save of {"image_proj": {...}, "ip_adapter": {...}},
read with weights_only=True). Refused, naming the key: a block count other than L2 + L1, biases on to_k_ip / to_v_ip, wrong shapes,
n outside 1..128, E not a multiple of 64 (rt_gemm_bf16 needs K % 64 == 0, and 2E is the second projection's K), unknown keys.
The image encoder this adapter is trained with (SigLIP-so400m) is image_encoder.SiglipVisionModel: ``ip_adapter_image=`` runs it and takes
its 1152-wide ``pooler_output``; an embedding computed elsewhere still comes in through ``ip_adapter_image_embeds=``.
"""
from __future__ import annotations

import itertools
import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import ops

_VERSIONS = itertools.count(1)     # IPAdapter.version: one number per set of device tensors (a captured graph holds their pointers)
MAX_TOKENS = 128                   # rt_ip_attention: 1 <= n_ip <= 128
DEFAULT_WEIGHT_NAME = "ip_adapter.safetensors"

# layout name -> (projection prefix, norm prefix, regex of a block key -> (block index, "k" | "v", "weight" | "bias"))
_LAYOUTS = {
    "diffusers": ("image_proj.proj", "image_proj.norm", re.compile(r"^ip_adapter\.(\d+)\.to_(k|v)_ip\.(weight|bias)$")),
    "xlabs": ("ip_adapter_proj_model.proj", "ip_adapter_proj_model.norm",
              re.compile(r"^double_blocks\.(\d+)\.processor\.ip_adapter_double_stream_(k|v)_proj\.(weight|bias)$")),
}
_INSTANTX_MARK = "image_proj.proj.0.weight"
_INSTANTX_BLOCK = re.compile(r"^ip_adapter\.(\d+)\.to_(k|v)_ip\.(weight|bias)$")
GEMM_K = 64                        # rt_gemm_bf16: K % 64 == 0
_SINGLE_BLOCK_KEYS = re.compile(r"(^|\.)single_(transformer_)?blocks\.|ip_adapter_single_stream")


@dataclass
class IPAdapterWeights:
    """Parsed checkpoint: tensors as stored in the file (any float dtype), one entry per double block — per block, double blocks
    first, for the "instantx" layout, whose projection has two layers (proj_w/proj_b the first, proj2_w/proj2_b the second) and
    whose K/V linears have no bias (k_b / v_b stay empty)."""

    proj_w: torch.Tensor            # [n·C, E]                       instantx: [2E, E]
    proj_b: torch.Tensor            # [n·C]                          instantx: [2E]
    norm_w: torch.Tensor            # [C]
    norm_b: torch.Tensor            # [C]
    k_w: List[torch.Tensor]         # [d, C] each
    k_b: List[torch.Tensor]
    v_w: List[torch.Tensor]
    v_b: List[torch.Tensor]
    num_tokens: int
    layout: str = "diffusers"       # "diffusers" | "xlabs" | "instantx"
    proj2_w: Optional[torch.Tensor] = None      # instantx: [n·C, 2E]
    proj2_b: Optional[torch.Tensor] = None
    num_double: int = 0             # instantx: blocks [0, num_double) are double blocks


def read_ip_adapter_file(path_or_dict, subfolder: Optional[str] = None, weight_name: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """State dict from a dict, a ``.safetensors`` file, a ``torch.save``d ``.bin`` / ``.pt`` file (read with weights_only=True), or a
    directory / cached hub id (+ ``subfolder``) with ``weight_name`` (lora.read_lora_file's resolution; nothing is fetched). The
    nested upstream form {"image_proj": {...}, "ip_adapter": {...}} is flattened with those two prefixes."""
    from . import lora

    def flat(sd):
        if sd and all(isinstance(v, dict) for v in sd.values()):
            return {f"{pre}.{k}": v for pre, inner in sd.items() for k, v in inner.items()}
        return dict(sd)

    if isinstance(path_or_dict, dict):
        return flat(path_or_dict)
    path = str(path_or_dict)
    if not os.path.isfile(path):
        from .modules import resolve_model_path

        path = resolve_model_path(path)
        if subfolder:
            path = os.path.join(path, subfolder)
        if weight_name is None:
            files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors")) if os.path.isdir(path) else []
            if DEFAULT_WEIGHT_NAME in files:
                weight_name = DEFAULT_WEIGHT_NAME
            elif len(files) == 1:
                weight_name = files[0]
            else:
                raise ValueError(f"{path}: pass weight_name= (no {DEFAULT_WEIGHT_NAME} and {len(files)} .safetensors files to choose from)")
        if not os.path.isfile(os.path.join(path, weight_name)):
            raise OSError(f"IP-Adapter file {os.path.join(path, weight_name)} not found")
        path = os.path.join(path, weight_name)
    if path.endswith((".bin", ".pt", ".pth")):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(sd, dict):
            raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
        return flat(sd)
    return lora.read_lora_file(path)[0]


def _parse_instantx(sd: Dict[str, torch.Tensor], num_layers: int, num_single_layers: int, C: int, d: int) -> IPAdapterWeights:
    pp, npfx = "image_proj.proj", "image_proj.norm"
    head = [f"{pp}.0.weight", f"{pp}.0.bias", f"{pp}.2.weight", f"{pp}.2.bias", f"{npfx}.weight", f"{npfx}.bias"]
    L = num_layers + num_single_layers
    blocks: Dict[int, Dict[str, torch.Tensor]] = {}
    for k in sd:
        if k in head:
            continue
        m = _INSTANTX_BLOCK.match(k)
        if m is None:
            raise ValueError(f"unrecognised IP-Adapter key: {k}")
        if m.group(3) == "bias":
            raise ValueError(f"the InstantX layout has no bias on to_k_ip / to_v_ip: {k}")
        blocks.setdefault(int(m.group(1)), {})[m.group(2)] = sd[k]
    for k in head:
        if k not in sd:
            raise ValueError(f"IP-Adapter state dict lacks {k}")
    if sorted(blocks) != list(range(L)):
        odd = next((i for i in sorted(blocks) if i >= L), None)
        i = odd if odd is not None else next(i for i in range(L) if i not in blocks)
        raise ValueError(f"IP-Adapter has {len(blocks)} blocks, the transformer {num_layers} double + {num_single_layers} single = {L} "
                         f"blocks: ip_adapter.{i}.to_k_ip.weight")
    w0, b0, w2, b2, norm_w, norm_b = (sd[k] for k in head)
    if norm_w.dim() != 1 or norm_w.shape[0] != C or norm_b.shape != norm_w.shape:
        raise ValueError(f"{npfx}.weight: width {tuple(norm_w.shape)} != joint_attention_dim {C}")
    if w0.dim() != 2 or w0.shape[0] != 2 * w0.shape[1]:
        raise ValueError(f"{pp}.0.weight: shape {tuple(w0.shape)} is not [2E, E]")
    E = w0.shape[1]
    if E % GEMM_K:
        raise ValueError(f"{pp}.0.weight: image embedding width {E} is not a multiple of {GEMM_K} (rt_gemm_bf16 needs K % {GEMM_K} == 0; "
                         f"E and 2E are the K of the two projections)")
    if b0.shape != (2 * E,):
        raise ValueError(f"{pp}.0.bias: shape {tuple(b0.shape)} does not match {pp}.0.weight")
    if w2.dim() != 2 or w2.shape[1] != 2 * E or w2.shape[0] % C or not 1 <= w2.shape[0] // C <= MAX_TOKENS:
        raise ValueError(f"{pp}.2.weight: shape {tuple(w2.shape)} is not 1..{MAX_TOKENS} tokens of width {C} from {2 * E} features")
    if b2.shape != (w2.shape[0],):
        raise ValueError(f"{pp}.2.bias: shape {tuple(b2.shape)} does not match {pp}.2.weight")
    out = IPAdapterWeights(w0, b0, norm_w, norm_b, [], [], [], [], w2.shape[0] // C, "instantx", w2, b2, num_layers)
    for i in range(L):
        for kv, ws in (("k", out.k_w), ("v", out.v_w)):
            w = blocks[i].get(kv)
            if w is None:
                raise ValueError(f"IP-Adapter state dict lacks ip_adapter.{i}.to_{kv}_ip.weight")
            if w.shape != (d, C):
                raise ValueError(f"ip_adapter.{i}.to_{kv}_ip.weight: shape {tuple(w.shape)} != (inner_dim {d}, joint_attention_dim {C})")
            ws.append(w)
    return out


def parse_ip_adapter_state_dict(sd: Dict[str, torch.Tensor], num_layers: int, joint_attention_dim: int, inner_dim: int,
                                num_single_layers: int = 0) -> IPAdapterWeights:
    """Any key layout -> IPAdapterWeights; every refusal names the offending key."""
    keys = list(sd)
    if _INSTANTX_MARK in sd:
        return _parse_instantx(sd, num_layers, num_single_layers, joint_attention_dim, inner_dim)
    bad = [k for k in keys if _SINGLE_BLOCK_KEYS.search(k)]
    if bad:
        raise ValueError(f"IP-Adapter keys that name single blocks are not supported (the InstantX file numbers all its blocks "
                         f"ip_adapter.{{j}}): {sorted(bad)[0]}")
    layout = next((name for name, (pp, _, rx) in _LAYOUTS.items() if any(k.startswith(pp + ".") or rx.match(k) for k in keys)), None)
    if layout is None:
        raise ValueError(f"no IP-Adapter keys found (expected image_proj.* / ip_adapter.* or ip_adapter_proj_model.* / double_blocks.*): "
                         f"{sorted(keys)[0] if keys else '<empty state dict>'}")
    pp, npfx, rx = _LAYOUTS[layout]
    head = {f"{pp}.weight", f"{pp}.bias", f"{npfx}.weight", f"{npfx}.bias"}
    blocks: Dict[int, Dict[Tuple[str, str], torch.Tensor]] = {}
    for k in keys:
        if k in head:
            continue
        m = rx.match(k)
        if m is None:
            raise ValueError(f"unrecognised IP-Adapter key: {k}")
        blocks.setdefault(int(m.group(1)), {})[(m.group(2), m.group(3))] = sd[k]
    for k in sorted(head):
        if k not in sd:
            raise ValueError(f"IP-Adapter state dict lacks {k}")

    def block_key(i, kv, part):
        return (f"ip_adapter.{i}.to_{kv}_ip.{part}" if layout == "diffusers"
                else f"double_blocks.{i}.processor.ip_adapter_double_stream_{kv}_proj.{part}")

    if sorted(blocks) != list(range(num_layers)):
        odd = next((i for i in sorted(blocks) if i >= num_layers), None)
        name = block_key(odd, "k", "weight") if odd is not None else block_key(next(i for i in range(num_layers) if i not in blocks), "k", "weight")
        raise ValueError(f"IP-Adapter has {len(blocks)} blocks, the transformer {num_layers} double blocks: {name}")
    C, d = joint_attention_dim, inner_dim
    norm_w, norm_b, proj_w, proj_b = sd[f"{npfx}.weight"], sd[f"{npfx}.bias"], sd[f"{pp}.weight"], sd[f"{pp}.bias"]
    if norm_w.dim() != 1 or norm_w.shape[0] != C or norm_b.shape != norm_w.shape:
        raise ValueError(f"{npfx}.weight: width {tuple(norm_w.shape)} != joint_attention_dim {C}")
    if proj_w.dim() != 2 or proj_w.shape[0] % C or not 1 <= proj_w.shape[0] // C <= MAX_TOKENS:
        raise ValueError(f"{pp}.weight: {proj_w.shape[0]} output features are not 1..{MAX_TOKENS} tokens of width {C}")
    if proj_b.shape != (proj_w.shape[0],):
        raise ValueError(f"{pp}.bias: shape {tuple(proj_b.shape)} does not match {pp}.weight")
    if proj_w.shape[1] % 8:
        raise ValueError(f"{pp}.weight: image embedding width {proj_w.shape[1]} is not a multiple of 8")
    out = IPAdapterWeights(proj_w, proj_b, norm_w, norm_b, [], [], [], [], proj_w.shape[0] // C, layout)
    for i in range(num_layers):
        for kv, ws, bs in (("k", out.k_w, out.k_b), ("v", out.v_w, out.v_b)):
            w, b = blocks[i].get((kv, "weight")), blocks[i].get((kv, "bias"))
            if w is None:
                raise ValueError(f"IP-Adapter state dict lacks {block_key(i, kv, 'weight')}")
            if b is None:
                raise ValueError(f"IP-Adapter state dict lacks {block_key(i, kv, 'bias')}")
            if w.shape != (d, C):
                raise ValueError(f"{block_key(i, kv, 'weight')}: shape {tuple(w.shape)} != (inner_dim {d}, joint_attention_dim {C})")
            if b.shape != (d,):
                raise ValueError(f"{block_key(i, kv, 'bias')}: shape {tuple(b.shape)} != ({d},)")
            ws.append(w)
            bs.append(b)
    return out


def normalize_scales(scale: Union[float, Sequence[float]], num_layers: int, per: str = "one per double block") -> List[float]:
    """set_ip_adapter_scale's argument -> one float per block the adapter has a term in."""
    if isinstance(scale, (int, float)):
        return [float(scale)] * num_layers
    s = [float(x) for x in scale]
    if len(s) != num_layers:
        raise ValueError(f"set_ip_adapter_scale: expected a float or {num_layers} floats ({per}), got {len(s)}")
    return s


def normalize_embeds(embeds) -> torch.Tensor:
    """``ip_adapter_image_embeds`` as given (tensor or one-element list; [B,1,E], [1,1,E], [B,E] or [1,E]) -> [B or 1, E]."""
    if isinstance(embeds, (list, tuple)):
        if len(embeds) != 1:
            raise ValueError(f"ip_adapter_image_embeds: one IP-Adapter is supported, got a list of {len(embeds)}")
        embeds = embeds[0]
    if not isinstance(embeds, torch.Tensor):
        raise TypeError(f"ip_adapter_image_embeds: expected a tensor or a one-element list, got {type(embeds)}")
    if embeds.dim() == 3:
        if embeds.shape[1] != 1:
            raise ValueError(f"ip_adapter_image_embeds: one image per sample is supported, got {embeds.shape[1]}")
        embeds = embeds[:, 0]
    if embeds.dim() != 2:
        raise ValueError(f"ip_adapter_image_embeds: expected [B,1,E] or [B,E], got {tuple(embeds.shape)}")
    return embeds


@dataclass
class PreparedIP:
    """Loop-invariant K/V of one call: per double block (K_i, V_i) [B or 1, n, d] bf16 views of one GEMM output, and the scales.
    ``inside`` = the InstantX form: one entry per block (``num_double`` double blocks, then the single blocks), the term goes inside
    the block (mmdit.run_double / run_single, ``ip_inside``)."""

    kv: List[Tuple[torch.Tensor, torch.Tensor]]
    scales: List[float]
    buf: torch.Tensor               # the storage the views point into
    inside: bool = False
    num_double: int = 0
    tok: Optional[torch.Tensor] = None   # InstantX form: the image tokens [B or 1, n, C] K/V were made from
    # a regional term (``regional_ip_weights``): fp32 weight per query row of a double block [B or 1, N] and of a single block
    # [B or 1, T + N]; None = every row at full strength, the launch without a table
    rows_img: Optional[torch.Tensor] = None
    rows_joint: Optional[torch.Tensor] = None

    def block_terms(self, j: int, single: bool = False) -> list:
        """This term as block j takes it in a list of terms: [(K, V, scale, row weights)], empty where its scale is zero."""
        if self.scales[j] == 0.0:
            return []
        return [(*self.kv[j], self.scales[j], self.rows_joint if single else self.rows_img)]


def regional_ip_weights(mask, scale: float = 1.0, *, N: int, batch: int = 1, cfg: bool = False, line: bool = False):
    """The one rule for the row weights of a regional image prompt, from host values alone -> (image rows [R, N] fp32, text rows [R]
    fp32), or (None, None) for the call's own image prompt without a mask (the unweighted launch).
    ``mask``: the term's region after the pipeline's ÷16 bilinear resize (fractional at the edges), as [N], [1, N, 1] or [batch, N, 1]
    values. ``scale``: the term's scalar (1.0 for the call's own prompt, ``control_ip_adapter_scale`` for a text line), folded into the
    weights. Image row n weighs scale · m[n]; the T text rows of an InstantX single block all weigh scale · mean_n m[n] (a full mask: the
    unmasked call; an empty one: nothing; a small box: its share of the area). R = 1 or ``batch`` as the mask is; under true CFG
    (``cfg``) the conditioning batch is [negative, positive] and R = 2 · batch: the call's own prompt (``line`` False) carries its mask
    in both halves, a text line's term weighs 0 everywhere in the negative half, which does not see the lines."""
    if mask is None:
        if line:
            raise ValueError("a text line's image prompt needs the line's regional mask")
        return None, None
    m = torch.as_tensor(mask).detach().to("cpu", torch.float32).reshape(-1, N)
    if m.shape[0] not in (1, batch):
        raise ValueError(f"regional image prompt: the mask has {m.shape[0]} entries for a batch of {batch}")
    img = m * float(scale)
    txt = m.mean(dim=1) * float(scale)
    if cfg:
        img, txt = img.expand(batch, N), txt.expand(batch)
        img = torch.cat([torch.zeros_like(img) if line else img, img])
        txt = torch.cat([torch.zeros_like(txt) if line else txt, txt])
    return img.contiguous(), txt.contiguous()


class IPAdapter:
    """Adapter state of one transformer: bf16 weights on the model's device, stacked [to_k_ip_0; to_v_ip_0; to_k_ip_1; ...] so that
    the K/V of every block come from ONE GEMM per call (M = B·n rows), and the per-block scales (default 1.0)."""

    _TENSORS = ("proj_w", "proj_b", "norm_scale", "norm_shift", "kv_w", "kv_b", "proj2_w", "proj2_b", "k_w", "v_w", "ones")

    def __init__(self, w: IPAdapterWeights, device):
        bf = lambda t: t.to(device=device, dtype=torch.bfloat16).contiguous()
        self.layout, self.num_double = w.layout, w.num_double
        self.num_tokens, self.num_layers = w.num_tokens, len(w.k_w)
        self.C, self.d, self.E = w.norm_w.shape[0], w.k_w[0].shape[0], w.proj_w.shape[1]
        self.proj_w, self.proj_b = bf(w.proj_w), bf(w.proj_b)
        self.scales = [1.0] * self.num_layers
        self.version = next(_VERSIONS)
        if w.layout == "instantx":
            # K and V of all L2 + L1 blocks come from ONE grouped launch: [to_k_ip_0; to_k_ip_1; ...] -> fp32 (normalised, then rounded)
            # and [to_v_ip_0; ...] -> bf16
            self.proj2_w, self.proj2_b = bf(w.proj2_w), bf(w.proj2_b)
            self.norm_scale = (bf(w.norm_w).to(torch.float32) - 1.0).contiguous()
            self.norm_shift = bf(w.norm_b).to(torch.float32).contiguous()
            self.k_w = torch.cat([bf(t) for t in w.k_w], dim=0).contiguous()          # [L·d, C]
            self.v_w = torch.cat([bf(t) for t in w.v_w], dim=0).contiguous()
            self.ones = torch.ones(128, device=device, dtype=torch.bfloat16)           # the weightless K norm through rt_rmsnorm_rows
            return
        # affine LayerNorm through rt_layernorm_modulate: LN(x)·(1 + scale) + shift with scale = weight - 1 (exact in fp32), shift = bias
        self.norm_scale = (bf(w.norm_w).to(torch.float32) - 1.0).contiguous()
        self.norm_shift = bf(w.norm_b).to(torch.float32).contiguous()
        self.kv_w = torch.cat([bf(t) for pair in zip(w.k_w, w.v_w) for t in pair], dim=0).contiguous()        # [L·2d, C]
        self.kv_b = torch.cat([bf(t) for pair in zip(w.k_b, w.v_b) for t in pair], dim=0).contiguous()

    def to_device(self, device) -> None:
        moved = False
        for name in self._TENSORS:
            old = getattr(self, name, None)
            if old is None:
                continue
            new = old.to(device)
            moved |= new is not old
            setattr(self, name, new)
        if moved:
            self.version = next(_VERSIONS)

    def set_scale(self, scale) -> None:
        if self.layout == "instantx":
            per = f"one per block: {self.num_double} double, then {self.num_layers - self.num_double} single"
            self.scales = normalize_scales(scale, self.num_layers, per)
        else:
            self.scales = normalize_scales(scale, self.num_layers)

    @property
    def active(self) -> bool:
        return any(s != 0.0 for s in self.scales)

    def prepare_terms(self, embeds: Sequence, weights: Optional[Sequence] = None, T: int = 0) -> List[PreparedIP]:
        """``prepare`` for several image prompts through this one adapter (regional terms): the embeddings [B_t or 1, E] are concatenated
        along the batch and projected ONCE (still three or six launches, M = the sum of their batches), and every term gets its rows of
        that one buffer as views. ``weights``: per term (image rows [R, N], text rows [R]) as ``regional_ip_weights`` returns them, or
        (None, None); ``T``: the text rows of a single block's query, which the InstantX form prepends to the image rows."""
        es = [normalize_embeds(e) for e in embeds]
        if not es:
            return []
        weights = [(None, None)] * len(es) if weights is None else list(weights)
        if len(weights) != len(es):
            raise ValueError(f"prepare_terms: {len(weights)} weight entries for {len(es)} image prompts")
        for e in es:
            if e.shape[1] != self.E:
                raise ValueError(f"ip_adapter_image_embeds: width {e.shape[1]} != the adapter's image embedding width {self.E}")
        dev = self.proj_w.device
        whole = self.prepare(es[0] if len(es) == 1 else torch.cat([e.to(device=dev, dtype=torch.bfloat16) for e in es], dim=0))
        out, o = [], 0
        for e, (img, txt) in zip(es, weights):
            rows = slice(o, o + e.shape[0])
            o += e.shape[0]
            ri = rj = None
            if img is not None:
                ri = img.to(device=dev, dtype=torch.float32).contiguous()
                if whole.inside:
                    rj = torch.cat([txt.to(device=dev, dtype=torch.float32)[:, None].expand(-1, T), ri], dim=1).contiguous()
            out.append(PreparedIP([(k[rows], v[rows]) for k, v in whole.kv], list(whole.scales), whole.buf, whole.inside, whole.num_double,
                                  None if whole.tok is None else whole.tok[rows], ri, rj))
        return out

    def prepare(self, embeds) -> PreparedIP:
        """Steps 1-2 for one call: three launches (projection GEMM, LayerNorm, stacked K/V GEMM); six for the InstantX form (two
        projection GEMMs with the exact GELU between them, LayerNorm, the stacked K and V GEMMs as one grouped launch, the K norm)."""
        e = normalize_embeds(embeds)
        if e.shape[1] != self.E:
            raise ValueError(f"ip_adapter_image_embeds: width {e.shape[1]} != the adapter's image embedding width {self.E}")
        if not self.proj_w.is_cuda:
            raise RuntimeError("the IP-Adapter is on the CPU; move the transformer to the GPU (there is no CPU fallback)")
        e = e.to(device=self.proj_w.device, dtype=torch.bfloat16).contiguous()
        B, n, C, d, L = e.shape[0], self.num_tokens, self.C, self.d, self.num_layers
        if self.layout == "instantx":
            f32 = lambda *shape: torch.empty(*shape, device=e.device, dtype=torch.float32)
            hid = ops.gelu_erf(ops.linear(e, self.proj_w, f32(B, 2 * self.E), bias=self.proj_b))
            t32 = ops.linear(hid, self.proj2_w, f32(B, n * C), bias=self.proj2_b)
            tok = torch.empty(B, n, C, device=e.device, dtype=torch.bfloat16)
            ops.layernorm_modulate(t32.view(B, n, C), tok, self.norm_shift.repeat(B, 1), self.norm_scale.repeat(B, 1), eps=1e-5)
            k32 = f32(B, n, L * d)
            kv = torch.empty(2, B, n, L * d, device=e.device, dtype=torch.bfloat16)
            ops.linear_grouped([ops.LinearProblem(tok, self.k_w, k32), ops.LinearProblem(tok, self.v_w, kv[1])])
            ops.rmsnorm_heads_(k32, kv[0], self.ones, eps=1e-5)
            views = [(kv[0][..., j * d : (j + 1) * d], kv[1][..., j * d : (j + 1) * d]) for j in range(L)]
            return PreparedIP(views, list(self.scales), kv, True, self.num_double, tok)
        t32 = torch.empty(B, n * C, device=e.device, dtype=torch.float32)
        ops.linear(e, self.proj_w, t32, bias=self.proj_b)
        tok = torch.empty(B, n, C, device=e.device, dtype=torch.bfloat16)
        ops.layernorm_modulate(t32.view(B, n, C), tok, self.norm_shift.repeat(B, 1), self.norm_scale.repeat(B, 1), eps=1e-5)
        kv = torch.empty(B, n, L * 2 * d, device=e.device, dtype=torch.bfloat16)
        ops.linear(tok, self.kv_w, kv, bias=self.kv_b)
        views = [(kv[..., 2 * i * d : (2 * i + 1) * d], kv[..., (2 * i + 1) * d : (2 * i + 2) * d]) for i in range(L)]
        return PreparedIP(views, list(self.scales), kv)
