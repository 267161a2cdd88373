"""FluxTransformer2DModel — the denoiser the reference imports from diffusers (PIPE:31) and calls at PIPE:1092-1104.

Not present under /root/reference; behaviour per SURVEY.md Appendix A.3. Same constructor config keys, same
``forward`` keyword names and return convention (``(sample,)`` when ``return_dict=False``), HIP kernels underneath.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Sequence, Any, Dict, List, Optional

import torch
import torch.nn as nn

from . import ip_adapter, lora, mmdit, ops
from .config import Config, flux_dev_transformer_config
from .modules import DoubleBlockParams, Lin, SingleBlockParams, TimeTextEmbedParams, WeightsIO, _ada
from .ops import LinearProblem as P


@dataclass
class Transformer2DModelOutput:
    sample: torch.Tensor


@dataclass
class StaticEmbeds:
    """Loop-invariant embeddings of one model for one call of the pipeline (``_MMDiTBase.prepare_static``): the prompt never
    changes between denoising steps and neither do the hint latents, so ``context_embedder(prompt)`` (A.3 / CN:292) and
    ``controlnet_x_embedder(cond)`` (CN:280) are evaluated once per image instead of once per step. Both are kept in the
    residual stream's dtype; adding them back is exact (same operands as the per-step path, fp32 addition commutes)."""

    ctx: torch.Tensor                     # [Bc, T, d]  context_embedder(encoder_hidden_states) + bias
    hint: Optional[torch.Tensor] = None   # [Bc, N, d]  controlnet_x_embedder(controlnet_cond) + bias (towers only)


class _MMDiTBase(nn.Module, WeightsIO):
    """Construction, planning and embedding steps common to the transformer and the ControlNet tower."""

    def _build_trunk(self, cfg: Config, device, dtype):
        kw = dict(device=device, dtype=dtype)
        d = cfg.num_attention_heads * cfg.attention_head_dim
        if cfg.attention_head_dim != 128:
            raise ValueError("the HIP attention kernels are specialised for attention_head_dim == 128")
        if sum(cfg.axes_dims_rope) != cfg.attention_head_dim:
            raise ValueError("sum(axes_dims_rope) must equal attention_head_dim")
        self.inner_dim = d
        self.time_text_embed = TimeTextEmbedParams(d, cfg.pooled_projection_dim, bool(cfg.guidance_embeds), **kw)
        self.context_embedder = Lin(cfg.joint_attention_dim, d, **kw)
        self.x_embedder = Lin(cfg.in_channels, d, **kw)
        self.transformer_blocks = nn.ModuleList([DoubleBlockParams(d, cfg.attention_head_dim, **kw) for _ in range(cfg.num_layers)])
        self.single_transformer_blocks = nn.ModuleList([SingleBlockParams(d, cfg.attention_head_dim, **kw) for _ in range(cfg.num_single_layers)])
        self._plans = None
        self._plan_key = None
        self._rope_cache = {}

    # ---- properties the pipelines read (PIPE:906)
    @property
    def dtype(self):
        return self.x_embedder.weight.dtype

    @property
    def device(self):
        return self.x_embedder.weight.device

    def random_init_(self, seed: int = 0, std: float = 0.02, bias_std: float = 0.02):
        """Synthetic weights for benchmarks (no checkpoints offline): W ~ N(0, std²), small biases, norm weights ≈ 1."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        for name, p in self.named_parameters():
            if name.endswith("norm_q.weight") or name.endswith("norm_k.weight") or name.endswith("norm_added_q.weight") or name.endswith("norm_added_k.weight"):
                p.data.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g, device=p.device, dtype=torch.float32))
            elif name.endswith(".bias"):
                p.data.copy_(bias_std * torch.randn(p.shape, generator=g, device=p.device, dtype=torch.float32))
            else:
                p.data.copy_(std * torch.randn(p.shape, generator=g, device=p.device, dtype=torch.float32))
        self._plans = None
        return self

    def _ensure_plans(self):
        """(Re)build fused weight views when parameters moved (``.to``) or were never planned."""
        key = (self.x_embedder.weight.data_ptr(), str(self.device), self.dtype)
        if self._plans is not None and self._plan_key == key:
            return self._plans
        if self.dtype != torch.bfloat16:
            raise TypeError(f"{type(self).__name__}: HIP path computes in bf16 storage; got {self.dtype}. Use torch_dtype=torch.bfloat16.")
        if not self.x_embedder.weight.is_cuda:
            raise RuntimeError(f"{type(self).__name__} is on {self.device}; move it to the GPU (.to('cuda')). There is no CPU fallback.")
        fp8, fa = getattr(self, "_fp8_linears", False), getattr(self, "_fp8_attention", False)
        self._plans = ([mmdit.plan_double(b, fp8, fa) for b in self.transformer_blocks], [mmdit.plan_single(b, fp8, fa) for b in self.single_transformer_blocks])
        self._plan_key = key
        self._rope_cache = {}
        return self._plans

    def _apply(self, fn, *a, **k):
        self._plans = None
        out = super()._apply(fn, *a, **k)
        if getattr(self, "_lora", None) is not None:
            self._lora.to_device(self.device)          # factors and W0 copies follow the weights
        if getattr(self, "_ip_adapter", None) is not None:
            self._ip_adapter.to_device(self.device)
        return out

    def enable_fp8_attention(self, on: bool = True):
        """BASELINE config 5 ("CDNA4 fp8 MFMA attention"): joint attention with e4m3 q, k, v and softmax numerators
        (rt_attention_fp8_prep / rt_attention_fp8_fwd; static quantisation, see csrc/attention_fp8.hip)."""
        self._fp8_attention = bool(on)
        self._plans = None
        return self

    def enable_fp8_linears(self, on=True):
        """BASELINE config 5 ("fp8 weights"): run the projections that read a LayerNorm output — to_q/k/v, add_q/k/v_proj,
        ff.net.0, ff_context.net.0, proj_mlp (58 % of the block's GEMM FLOPs) — on the e4m3 MFMA path. Weights are quantised
        per output channel when the plans are (re)built, activations per token inside the LayerNorm kernel; everything else
        (attention, out/down projections, residual stream, adaLN) is unchanged. Accuracy: e4m3 carries 3 mantissa bits —
        see DESIGN.md §4 for the measured floor. ``on="all"`` adds to_out / to_add_out, ff.net.2 and proj_out, whose bf16 inputs
        (attention output, GELU hidden) are quantised per token by one extra pass each. ``on="mx"``: the same projections, but
        those inputs carry one E8M0 scale per 32 elements (MX block scaling, applied by the MFMA's scale operand) and are written
        as e4m3 by the epilogue that computes them — the GELU hidden by the ff.net.0 / fused GEMM, the attention output by the
        e4m3 attention kernel (a block-quantise pass only when the bf16 attention kernel is in use): no separate passes."""
        if on not in (True, False, "ln", "all", "mx"):
            raise ValueError("enable_fp8_linears: True/'ln' (LayerNorm-fed projections), 'all' / 'mx' (every block projection), or False")
        self._fp8_linears = "ln" if on is True else on
        self._plans = None
        return self

    def load_state_dict(self, sd, strict: bool = True, **kw):
        if getattr(self, "_lora", None) is not None:
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: LoRA adapters are merged into the weights; unload_lora() first")
        out = super().load_state_dict(sd, strict=strict, **kw)
        if getattr(self, "_fp8_linears", False):
            self._plans = None          # the e4m3 copies of the weights are stale
        return out

    # ---- LoRA adapters: the PeftAdapterMixin subset (CN:22,41), merged into the bf16 weights on the device (lora.py)
    def _fp8_rows(self) -> Dict[str, tuple]:
        """{module path: (bf16 plan weight, e4m3 copy, row scales, r0, r1)} for every Linear whose weight is rows r0:r1 of a plan tensor
        with an e4m3 copy (enable_fp8_linears); built once per plan build."""
        plans = self._ensure_plans()
        cache = getattr(self, "_fp8_rows_cache", None)
        if cache is not None and cache[0] is plans:
            return cache[1]
        by_storage = {}
        for pl in list(plans[0]) + list(plans[1]):
            for full, w8, ws in mmdit.fp8_copies(pl):
                by_storage[full.untyped_storage().data_ptr()] = (full, w8, ws)
        rows = {}
        for name, mod in self.named_modules():
            hit = by_storage.get(mod.weight.data.untyped_storage().data_ptr()) if isinstance(mod, Lin) else None
            if hit is None:
                continue
            full, w8, ws = hit
            w = mod.weight.data
            r0, rem = divmod(w.data_ptr() - full.data_ptr(), full.stride(0) * full.element_size())
            r1 = r0 + w.shape[0]
            if rem or r0 < 0 or r1 > full.shape[0] or w.shape[1] != full.shape[1] or w.stride() != full.stride():
                raise RuntimeError(f"{name}: weight is not a row range of its fp8 plan tensor")
            rows[name] = (full, w8, ws, r0, r1)
        self._fp8_rows_cache = (plans, rows)
        return rows

    def _lora_unsupported(self, path: str, lin) -> Optional[str]:
        """Why a LoRA may not target this Linear (None: it may)."""
        if lin.in_features % 8:
            return f"in-features {lin.in_features} are not a multiple of 8"
        return None

    def state_dict(self, *args, **kwargs):
        """The weights at call scale 1.0: a call with joint_attention_kwargs={"scale": s} leaves the adapters merged at s until the
        next call or adapter change (lora.py), so a save between calls re-merges at 1.0 first."""
        if getattr(self, "_lora", None) is not None:
            self._lora.sync(1.0)
        return super().state_dict(*args, **kwargs)

    def _lora_manager(self) -> "lora.LoraManager":
        if getattr(self, "_lora", None) is None:
            raise ValueError(f"{type(self).__name__}: no LoRA adapter is loaded")
        return self._lora

    def load_lora_adapter(self, pretrained_model_name_or_path_or_dict, adapter_name: Optional[str] = None,
                          weight_name: Optional[str] = None, prefix: str = "transformer", **unused):
        """Read a diffusers/PEFT LoRA (dict, .safetensors file, directory or cached hub id), make it the only active adapter at
        weight 1.0 and merge it. ``adapter_name`` defaults to ``default_<n>``."""
        from . import lora

        sd, meta = lora.read_lora_file(pretrained_model_name_or_path_or_dict, weight_name)
        parsed = lora.parse_lora_state_dict(sd, meta, prefix)
        m = getattr(self, "_lora", None) or lora.LoraManager(self)
        m.load(adapter_name or f"default_{len(m.state.adapters)}", parsed)
        self._lora = m
        m.sync()
        return self

    def set_adapters(self, adapter_names, weights=None):
        m = self._lora_manager()
        m.state.set_adapters(adapter_names, weights)
        m.sync()

    def fuse_lora(self, lora_scale: float = 1.0, adapter_names=None, **unused):
        m = self._lora_manager()
        m.state.fuse(lora_scale, adapter_names)
        m.sync()

    def unfuse_lora(self):
        if getattr(self, "_lora", None) is not None:
            self._lora.state.unfuse()
            self._lora.sync()

    def unload_lora(self):
        """Drop every adapter. Unfused ones leave the weights (bit for bit the pre-LoRA weights when nothing is fused); fused ones stay
        baked in, as diffusers' fuse_lora() + unload_lora_weights() recipe expects. Factors and W0 copies are freed."""
        if getattr(self, "_lora", None) is not None:
            self._lora.unload()
            self._lora = None

    def delete_adapters(self, adapter_names):
        m = self._lora_manager()
        m.state.delete(adapter_names)
        m.sync()

    def disable_adapters(self):
        m = self._lora_manager()
        m.state.set_enabled(False)
        m.sync()

    def enable_adapters(self):
        m = self._lora_manager()
        m.state.set_enabled(True)
        m.sync()

    def active_adapters(self) -> List[str]:
        m = getattr(self, "_lora", None)
        return [] if m is None else [a for a, _ in m.state.active]

    def _apply_lora_scale(self, joint_attention_kwargs: Optional[Dict[str, Any]]) -> None:
        """CN:263-276: the call's LoRA scale (joint_attention_kwargs["scale"], 1.0 without one) merged before the call; nothing is
        launched when the weights already hold that state (e.g. inside the pipeline's loop, which applies it once up front)."""
        if getattr(self, "_lora", None) is not None:
            s = float((joint_attention_kwargs or {}).get("scale", 1.0))
            self._lora.sync(s)

    def _rope(self, txt_ids: torch.Tensor, img_ids: torch.Tensor):
        """cos/sin [S,128] fp32; constant over the denoising loop, so cached on the id tensors' identity."""
        if txt_ids.dim() == 3:
            txt_ids = txt_ids[0]
        if img_ids.dim() == 3:
            img_ids = img_ids[0]
        key = (txt_ids.data_ptr(), img_ids.data_ptr(), txt_ids.shape[0], img_ids.shape[0])
        hit = self._rope_cache.get(key)
        if hit is None:
            ids = torch.cat([txt_ids.to(torch.float32), img_ids.to(torch.float32)], dim=0)
            hit = ops.rope_table(ids, tuple(self.config.axes_dims_rope), 10000.0)
            if len(self._rope_cache) > 8:
                self._rope_cache.clear()
            self._rope_cache[key] = hit + (txt_ids, img_ids)   # keep the id tensors alive so data_ptr stays unique
        return hit[0], hit[1]

    def _embed_scalars(self, B, timestep, guidance):
        """(t·1000 [len(timestep) or B], g·1000 [B] or None) as fp32, the inputs of the sinusoidal embeddings (CN:282-284)."""
        ref16 = mmdit.REF_BF16_SCALARS
        t1000 = mmdit.bf16_round_trip_x1000(timestep.reshape(-1)) if ref16 else timestep.to(torch.float32).reshape(-1) * 1000.0
        if t1000.numel() == 1 and B > 1:
            t1000 = t1000.expand(B)
        g1000 = None
        if self.config.guidance_embeds:
            if guidance is None:
                raise ValueError("guidance_embeds=True requires `guidance`")
            g1000 = (mmdit.bf16_round_trip_x1000(guidance.reshape(-1)) if ref16 else guidance.to(torch.float32).reshape(-1) * 1000.0).contiguous()
            if g1000.numel() == 1 and B > 1:
                g1000 = g1000.expand(B).contiguous()
        return t1000.contiguous(), g1000

    def _temb(self, ws, timestep, guidance, pooled):
        t1000, g1000 = self._embed_scalars(ws.B, timestep, guidance)
        return mmdit.time_text_embed(self.time_text_embed, ws, t1000, g1000, pooled)

    def prepare_static(self, encoder_hidden_states: torch.Tensor, controlnet_cond: Optional[torch.Tensor] = None) -> StaticEmbeds:
        """See StaticEmbeds. ``controlnet_cond`` [Bc,N,in+extra] only for models that own a ``controlnet_x_embedder``."""
        self._ensure_plans()
        d = self.inner_dim
        xdt = torch.float32 if mmdit.RESIDUAL_F32 else torch.bfloat16
        e = encoder_hidden_states.to(torch.bfloat16).contiguous()
        ctx = torch.empty(e.shape[0], e.shape[1], d, device=e.device, dtype=xdt)
        ops.linear(e, self.context_embedder.weight.data, ctx, bias=self.context_embedder.bias.data)
        hint = None
        if controlnet_cond is not None:
            cond, cxw = self._padded_hint(controlnet_cond.to(torch.bfloat16))
            if cond.shape[0] != e.shape[0]:
                cond = cond.expand(e.shape[0], -1, -1) if cond.shape[0] == 1 else cond.repeat(e.shape[0] // cond.shape[0], 1, 1)
            hint = torch.empty(e.shape[0], cond.shape[1], d, device=e.device, dtype=xdt)
            ops.linear(cond.contiguous(), cxw, hint, bias=self.controlnet_x_embedder.bias.data)
        return StaticEmbeds(ctx, hint)

    def build_modulation_table(self, timesteps, guidance, pooled) -> "mmdit.ModulationTable":
        """adaLN vectors of every block for every entry of ``timesteps`` (model-scale values, i.e. t/1000 as the pipeline
        passes them, PIPE:1048,1094) — see mmdit.ModulationTable. guidance [B] / pooled [B,P] as in ``forward``."""
        doubles, singles = self._ensure_plans()
        B, d = pooled.shape[0], self.inner_dim
        dev = pooled.device
        # guidance and pooled text are the same at every step: their MLPs run once, the timestep MLP for all steps at once
        ts = torch.empty(len(timesteps) * B, device=dev, dtype=torch.float32)
        for i, t in enumerate(timesteps):                    # device fills (no host copy: this runs inside the loop's graph capture)
            ts[i * B : (i + 1) * B].fill_(float(t))
        t1000, g1000 = self._embed_scalars(B, ts, guidance)
        temb_all = mmdit.time_text_embed_all(self.time_text_embed, t1000, g1000, pooled, B)
        return mmdit.ModulationTable(temb_all, len(timesteps), B, doubles, singles, getattr(self, "norm_out", None) and self.norm_out.linear)

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=None, subfolder: Optional[str] = None, device=None, **unused):
        d = cls._resolve_dir(path, subfolder)
        cfg = Config.from_json_file(d + "/" + cls.config_name)
        model = cls(**cfg, device=device or "cpu", dtype=torch_dtype or torch.bfloat16)
        sd = cls._load_safetensors_dir(d)
        model.load_state_dict({k: v.to(torch_dtype or torch.bfloat16) for k, v in sd.items()}, strict=True)
        return model


class FluxTransformer2DModel(_MMDiTBase):
    def __init__(self, patch_size: int = 1, in_channels: int = 64, out_channels: Optional[int] = None, num_layers: int = 19,
                 num_single_layers: int = 38, attention_head_dim: int = 128, num_attention_heads: int = 24,
                 joint_attention_dim: int = 4096, pooled_projection_dim: int = 768, guidance_embeds: bool = False,
                 axes_dims_rope=(16, 56, 56), device=None, dtype=None):
        super().__init__()
        self.config = Config(patch_size=patch_size, in_channels=in_channels, out_channels=out_channels, num_layers=num_layers,
                             num_single_layers=num_single_layers, attention_head_dim=attention_head_dim,
                             num_attention_heads=num_attention_heads, joint_attention_dim=joint_attention_dim,
                             pooled_projection_dim=pooled_projection_dim, guidance_embeds=guidance_embeds,
                             axes_dims_rope=list(axes_dims_rope))
        self.out_channels = out_channels or in_channels
        self._build_trunk(self.config, device, dtype)
        d = self.inner_dim
        self.norm_out = _ada(d, 2, device=device, dtype=dtype)
        self.proj_out = Lin(d, patch_size * patch_size * self.out_channels, device=device, dtype=dtype)
        self._ip_adapter: Optional["ip_adapter.IPAdapter"] = None

    # ---- IP-Adapter (image prompt): the FluxIPAdapterMixin subset; state in ip_adapter.py, not in the parameters
    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder: Optional[str] = None, weight_name: Optional[str] = None):
        """Read an IP-Adapter (dict, .safetensors file, directory + weight_name, or cached hub id; diffusers, XLabs or InstantX key
        layout, the last also as its upstream ``ip-adapter.bin``) and make it this model's adapter at scale 1.0 in every block it has
        a term in: the double blocks, for the InstantX layout the single blocks too. Replaces a loaded one."""
        sd = ip_adapter.read_ip_adapter_file(pretrained_model_name_or_path_or_dict, subfolder, weight_name)
        w = ip_adapter.parse_ip_adapter_state_dict(sd, self.config.num_layers, self.config.joint_attention_dim, self.inner_dim,
                                                   self.config.num_single_layers)
        self._ip_adapter = ip_adapter.IPAdapter(w, self.device)
        return self

    def set_ip_adapter_scale(self, scale):
        """One float for every block of the adapter, or a list: num_layers floats (diffusers / XLabs layouts), num_layers +
        num_single_layers floats, double blocks first (InstantX layout). A block at 0.0 launches nothing for the adapter."""
        if self._ip_adapter is None:
            raise ValueError(f"{type(self).__name__}: no IP-Adapter is loaded")
        self._ip_adapter.set_scale(scale)

    def unload_ip_adapter(self):
        self._ip_adapter = None

    @torch.no_grad()
    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor = None,
                pooled_projections: torch.Tensor = None, timestep: torch.Tensor = None, img_ids: torch.Tensor = None,
                txt_ids: torch.Tensor = None, guidance: torch.Tensor = None,
                joint_attention_kwargs: Optional[Dict[str, Any]] = None, controlnet_block_samples=None,
                controlnet_single_block_samples=None, return_dict: bool = True, controlnet_blocks_repeat: bool = False,
                _mods: Optional["mmdit.StepMods"] = None, _sample_events: Optional[Sequence["torch.cuda.Event"]] = None,
                _static: Optional[StaticEmbeds] = None, _ip: Optional["ip_adapter.PreparedIP"] = None,
                _groups: Optional["ops.KeyGroups"] = None, _key_bias: Optional[torch.Tensor] = None, _perturbed=None):
        """``joint_attention_kwargs["ip_adapter_image_embeds"]`` (as in diffusers): the image prompt of a loaded IP-Adapter, projected
        and applied in every double block — in every block, single ones included, for an InstantX adapter (ip_adapter.py); ``_ip`` (optional) = the same already prepared (``_ip_adapter.prepare``), so
        that a loop does not redo the projection per step, or a list of them (``_ip_adapter.prepare_terms``): regional image prompts, of which
        block j gets, in order, those whose scale on block j is not zero (they share the adapter's per-block scales).
        ``_sample_events[k]`` (optional): event another stream records when controlnet_block_samples[k] is complete; the
        current stream waits for it right before the first block that consumes that sample. ``_static`` (optional): this
        model's loop-invariant embeddings (prepare_static) — the text rows are copied instead of recomputed. ``_groups`` (optional): an
        ops.KeyGroups over the T + N joint rows, handed to the joint attention of every block (per-line prompts, pipeline.line_prompt_groups); ``_key_bias``
        (optional, with ``_groups``): fp32 [Bc or 1, 32], a bias per key group or class for the same launches (pipeline.line_prompt_bias).
        ``_perturbed`` (optional, not with ``_groups``): a pipeline.Perturbed — perturbed-attention guidance: the double blocks in its
        ``double_ids`` and the single blocks in its ``single_ids`` alone run their joint attention under its tables with the self rule
        (ops.attention(self_key=True)); every other block is called as without it."""
        doubles, singles = self._ensure_plans()
        joint_attention_kwargs = dict(joint_attention_kwargs or {})          # a copy: the image prompt is popped below, as diffusers does
        ip_embeds = joint_attention_kwargs.pop("ip_adapter_image_embeds", None)
        self._apply_lora_scale(joint_attention_kwargs)
        cfg = self.config
        B, N, _ = hidden_states.shape
        Bc = encoder_hidden_states.shape[0]       # conditioning batch may be a multiple of B (inpaint CFG, Q6)
        T = encoder_hidden_states.shape[1]
        H, d = cfg.num_attention_heads, self.inner_dim
        ws = mmdit.workspace(Bc, T, N, d, hidden_states.device, need_single=len(singles) > 0)
        hs = hidden_states.to(torch.bfloat16)
        if Bc != B:
            if Bc % B:
                raise ValueError("conditioning batch must be a multiple of the latent batch")
            hs = hs.repeat(Bc // B, 1, 1)
        if _static is not None:
            ws.x[:, :T].copy_(_static.ctx)                                   # device copy of the loop-invariant text rows
            ops.linear(hs.contiguous(), self.x_embedder.weight.data, ws.x[:, T:], bias=self.x_embedder.bias.data)
        else:
            ops.linear_grouped([P(hs.contiguous(), self.x_embedder.weight.data, ws.x[:, T:], bias=self.x_embedder.bias.data),
                                P(encoder_hidden_states.to(torch.bfloat16).contiguous(), self.context_embedder.weight.data, ws.x[:, :T],
                                  bias=self.context_embedder.bias.data)])
        temb = None if _mods is not None else self._temb(ws, timestep, guidance, pooled_projections)
        cos, sin = self._rope(txt_ids, img_ids)
        nl, ns = len(doubles), len(singles)
        if _ip is None and ip_embeds is not None:
            if getattr(self, "_ip_adapter", None) is None:
                raise ValueError("ip_adapter_image_embeds were passed but no IP-Adapter is loaded (load_ip_adapter)")
            _ip = self._ip_adapter.prepare(ip_embeds) if self._ip_adapter.active else None
        ip_list = _ip if isinstance(_ip, (list, tuple)) else None          # regional terms; a single PreparedIP takes the lines it always took
        if ip_list is not None:
            _ip = ip_list[0] if ip_list else None
        waited = set()
        gkw = {} if _groups is None else dict(groups=_groups)               # a call without key groups calls the blocks as it always did
        if _key_bias is not None:
            gkw["key_bias"] = _key_bias
        pkw, p_double, p_single = {}, frozenset(), frozenset()
        if _perturbed is not None:
            if _groups is not None:
                raise ValueError("_perturbed and _groups cannot be combined (one set of tables per attention launch)")
            pkw = dict(groups=_perturbed.groups(), self_key=True)
            p_double, p_single = _perturbed.double_ids, _perturbed.single_ids
        for i, pl in enumerate(doubles):
            inj = None
            if controlnet_block_samples is not None:
                ns_c = len(controlnet_block_samples)
                k = i % ns_c if controlnet_blocks_repeat else i // int(math.ceil(nl / ns_c))
                inj = controlnet_block_samples[k]
                if _sample_events is not None and k not in waited:
                    torch.cuda.current_stream().wait_event(_sample_events[k])
                    waited.add(k)
            ip = None if _ip is None or _ip.scales[i] == 0.0 else (*_ip.kv[i], _ip.scales[i])
            if ip_list is not None:
                ip = [t for p in ip_list for t in p.block_terms(i)] or None
            mmdit.run_double(pl, ws, temb, cos, sin, H, inject=inj, mods=None if _mods is None else _mods.double[i], ip=ip,
                             ip_inside=_ip is not None and _ip.inside, **(pkw if i in p_double else gkw))
        for i, pl in enumerate(singles):
            inj = None
            if controlnet_single_block_samples is not None:
                inj = controlnet_single_block_samples[i // int(math.ceil(ns / len(controlnet_single_block_samples)))]
            ip = None
            if _ip is not None and _ip.inside and _ip.scales[nl + i] != 0.0:
                ip = (*_ip.kv[nl + i], _ip.scales[nl + i])
            if ip_list is not None and _ip is not None and _ip.inside:
                ip = [t for p in ip_list for t in p.block_terms(nl + i, single=True)] or None
            mmdit.run_single(pl, ws, temb, cos, sin, H, inject=inj, mods=None if _mods is None else _mods.single[i], ip=ip,
                             **(pkw if i in p_single else gkw))
        # AdaLayerNormContinuous: chunk order (scale, shift)  — A.3
        if _mods is not None:
            m = _mods.out
        else:
            m = ws.mod_a[:, : 2 * d]
            ops.gemv(temb, self.norm_out.linear.weight.data, self.norm_out.linear.bias.data, m, silu_in=True)
        ops.layernorm_modulate(ws.x[:, T:], ws.xn[:, T:], m[:, d : 2 * d], m[:, :d])
        out = torch.empty(Bc, N, self.proj_out.weight.shape[0], device=hs.device, dtype=torch.bfloat16)
        ops.linear(ws.xn[:, T:], self.proj_out.weight.data, out, bias=self.proj_out.bias.data)
        if not return_dict:
            return (out,)
        return Transformer2DModelOutput(sample=out)
