"""What the four encoders that run before the denoising loop share (text_encoders.py: T5, CLIP text; image_encoder.py: CLIP vision,
SigLIP): the parameter holders, the ``_Encoder`` base (dtype / device, plans, ``from_pretrained``), the pre-LN transformer stack of the
three CLIP / SigLIP models (``_PreLNStack``) and the per-head assembled attention for heads of 64 with a bias.

One rule for the plans, the one mmdit.py follows: a plan holds VIEWS of the parameters and nothing computed from their values. Weights
a GEMM reads as one operand (q|k|v, T5's wi_1|wi_0) are fused in place by ``modules._fuse``; weights the GEMM needs zero-padded are moved
into the padded tensor the same way (``_mlp_padded``). So no weight is held twice, and a write into a parameter is seen by the next
forward. The few small tensors that ARE computed from parameter values (the LayerNorm vectors in fp32: ``_Affines``; position tables)
are computed by every ``forward``, in a handful of launches for the whole model.
"""
from __future__ import annotations

import json
import os
from typing import Optional

import torch
import torch.nn as nn

from . import native, ops
from .ops import _dev, _opt
from .modules import WeightsIO, _fuse

BF16, F32 = torch.bfloat16, torch.float32


class _H(nn.Module):
    pass


class _W(nn.Module):
    """weight-only parameter holder (bias-free Linear / T5LayerNorm / Embedding)."""

    def __init__(self, *shape, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*shape, device=device, dtype=dtype), requires_grad=False)


class _WB(nn.Module):
    def __init__(self, out_f, in_f=None, device=None, dtype=None):
        super().__init__()
        shape = (out_f,) if in_f is None else (out_f, in_f)
        self.weight = nn.Parameter(torch.empty(*shape, device=device, dtype=dtype), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_f, device=device, dtype=dtype), requires_grad=False)


def _stream():
    return ops._stream()


def _encoder_layers(n: int, d: int, F_: int, kw: dict) -> nn.Module:
    """``encoder.layers.*`` of the three transformers classes: self_attn.{q,k,v,out}_proj, layer_norm1/2, mlp.fc1/fc2."""
    enc = _H()
    enc.layers = nn.ModuleList()
    for _ in range(n):
        l = _H()
        sa = _H()
        sa.q_proj, sa.k_proj, sa.v_proj, sa.out_proj = (_WB(d, d, **kw) for _ in range(4))
        l.self_attn = sa
        l.layer_norm1, l.layer_norm2 = _WB(d, **kw), _WB(d, **kw)
        mlp = _H()
        mlp.fc1, mlp.fc2 = _WB(F_, d, **kw), _WB(d, F_, **kw)
        l.mlp = mlp
        enc.layers.append(l)
    return enc


class _Affines:
    """The LayerNorms of a model as constant vectors of the adaLN kernel: LayerNorm(x)·w + b == LN(x)·(1 + (w - 1)) + b. The kernel
    reads them in fp32, so these are the one thing a plan computes from parameter values: the holders' parameters are fused in place
    and ``refresh``, called by every forward, recomputes all vectors from what the parameters hold now in three launches.
    ``refresh()[holder]`` is that LayerNorm's (w - 1, b) as f32 [1,d] rows."""

    def __init__(self, norms):
        self.w, self.b = _fuse(norms)                                            # bf16 [n·d] each
        n = len(norms)
        self.scale, self.shift = (torch.empty(n, self.w.numel() // n, device=self.w.device, dtype=F32) for _ in range(2))
        self.rows = {m: (self.scale[i : i + 1], self.shift[i : i + 1]) for i, m in enumerate(norms)}

    def refresh(self) -> dict:
        self.scale.copy_(self.w.view_as(self.scale)).sub_(1.0)
        self.shift.copy_(self.b.view_as(self.shift))
        return self.rows


def pad_mlp_to_64(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor):
    """(fc1.weight [F,d], fc1.bias [F], fc2.weight [d,F]) with F padded by zeros to the next multiple of 64 (the GEMM's K % 64 rule
    for fc2: 4304 -> 4352). Exact: a padded hidden unit is gelu_tanh(0·x + 0) = 0 and meets a zero column of fc2."""
    F_ = w1.shape[0]
    Fp = (F_ + 63) // 64 * 64
    if Fp == F_:
        return w1.contiguous(), b1.contiguous(), w2.contiguous()
    w1p = torch.zeros(Fp, w1.shape[1], device=w1.device, dtype=w1.dtype)
    w1p[:F_] = w1
    b1p = torch.zeros(Fp, device=b1.device, dtype=b1.dtype)
    b1p[:F_] = b1
    w2p = torch.zeros(w2.shape[0], Fp, device=w2.device, dtype=w2.dtype)
    w2p[:, :F_] = w2
    return w1p, b1p, w2p


def _mlp_padded(mlp) -> tuple:
    """(w1, b1, w2, b2) of an ``mlp.fc1`` / ``mlp.fc2`` pair, padded by ``pad_mlp_to_64``; the three padded parameters are re-pointed at
    the unpadded part of the padded tensors, as ``_fuse`` re-points what it concatenates (the identity when F % 64 == 0)."""
    F_ = mlp.fc1.weight.shape[0]
    w1, b1, w2 = pad_mlp_to_64(mlp.fc1.weight.data, mlp.fc1.bias.data, mlp.fc2.weight.data)
    mlp.fc1.weight.data, mlp.fc1.bias.data, mlp.fc2.weight.data = w1[:F_], b1[:F_], w2[:, :F_]
    return w1, b1, w2, mlp.fc2.bias.data


def _quick_gelu(hid: torch.Tensor) -> None:
    native.call("rt_quick_gelu", _dev(hid, "hid", BF16), hid.numel(), _stream())


def _attention_heads(q, k, v, out, H, bias, scale, T, Tp, scratch):
    """out[b, :, h*64:(h+1)*64] = softmax(scale * q_h k_hᵀ + bias[h or 0]) v_h for every (batch, head).

    q, k, v, out: [B, Tp, H*64] bf16 views (row stride = their own ld); bias f32 [Hb, T, T] with Hb in (1, H) or None.
    Tp = T rounded up to 64 (rows/keys >= T are padding: keys masked by writing zero probabilities, rows ignored)."""
    B = q.shape[0]
    scores, probs, vt = scratch
    for b in range(B):
        for h in range(H):
            qh, kh, vh = q[b, :, h * 64 : (h + 1) * 64], k[b, :, h * 64 : (h + 1) * 64], v[b, :, h * 64 : (h + 1) * 64]
            ops.linear(qh, kh, scores)                                           # [Tp, Tp] f32 = q_h k_hᵀ
            bh = None if bias is None else bias[h if bias.shape[0] > 1 else 0]
            native.call("rt_softmax_rows_bias", _dev(scores, "scores", F32), Tp, _opt(bh, "bias", F32), 0 if bh is None else bh.stride(0),
                        _dev(probs, "probs", BF16), Tp, T, T, Tp, float(scale), _stream())
            native.call("rt_transpose_bf16", _dev(vh, "v", BF16), _dev(vt, "vt", BF16), Tp, 64, vh.stride(0), Tp, _stream())
            ops.linear(probs, vt, out[b, :, h * 64 : (h + 1) * 64])              # [Tp, 64] = P v_h


def _attention_scratch(Tp: int, device) -> tuple:
    """The ``scratch`` of ``_attention_heads``: scores [Tp,Tp] f32, probabilities [Tp,Tp] bf16 and vᵀ [64,Tp] bf16. The probabilities
    start as zeros and only rows and keys < T are ever written, so padded query rows and keys keep zero probabilities."""
    return (torch.empty(Tp, Tp, device=device, dtype=F32), torch.zeros(Tp, Tp, device=device, dtype=BF16),
            torch.empty(64, Tp, device=device, dtype=BF16))


class _Encoder(nn.Module, WeightsIO):
    """Base of the four encoders; it holds no parameters of its own. A class names the parameter its dtype and device are read from
    (``_anchor``) and the section of ``config.json`` that holds its constructor arguments when the file describes a two-tower model
    (``_config_section``), builds its modules, and implements ``_build_plans``, ``load_state_dict`` (its own key rewriting, then
    ``_load``) and ``forward``."""

    config_name = "config.json"
    weights_name = "model.safetensors"
    _anchor: str
    _config_section: Optional[str] = None
    _plans = None

    @property
    def dtype(self):
        return self.get_parameter(self._anchor).dtype

    @property
    def device(self):
        return self.get_parameter(self._anchor).device

    def _reset_plans(self):
        """The one hook for everything that may replace a parameter's storage."""
        self._plans = None

    def _apply(self, fn, *a, **k):
        self._reset_plans()
        return super()._apply(fn, *a, **k)

    def _load(self, sd, strict, **kw):
        self._reset_plans()
        return nn.Module.load_state_dict(self, {k: v for k, v in sd.items() if not k.endswith("position_ids")}, strict=strict, **kw)

    def _ensure_plans(self):
        if self._plans is None:
            if self.dtype != BF16 or self.device.type != "cuda":
                raise RuntimeError(f"{type(self).__name__} (HIP): bf16 on the GPU only; there is no CPU fallback")
            self._plans = self._build_plans()
        return self._plans

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=None, subfolder: Optional[str] = None, device=None, **unused):
        d = cls._resolve_dir(path, subfolder)
        with open(os.path.join(d, cls.config_name)) as f:
            cfg = json.load(f)
        cfg = {k: v for k, v in cfg.get(cls._config_section, cfg).items() if k not in ("dtype", "device")}    # transformers 5.x records a dtype
        m = cls(**cfg, device=device or "cpu", dtype=torch_dtype or BF16)
        m.load_state_dict({k: v.to(torch_dtype or BF16) for k, v in cls._load_safetensors_dir(d).items()}, strict=True)
        return m


class _PreLNStack(_Encoder):
    """The pre-LN transformer layers of CLIP text, CLIP vision and SigLIP (``_encoder_layers``): their plans and the layer loop. A class
    sets its head dim (``_head_dim``: which of the two small-head attention entry points the layers call), or takes the assembled
    attention from ``_AssembledAttention``."""

    _head_dim: int

    def _layer_plans(self, layers) -> dict:
        """Per layer (wqkv, bqkv, wo, bo, w1, b1, w2, b2, layer_norm1, layer_norm2): weight views, and the two LayerNorm holders as
        keys into ``plans["norms"]``, the ``_Affines`` of every LayerNorm of the model."""
        plan = []
        for l in layers:
            sa = l.self_attn
            plan.append(_fuse([sa.q_proj, sa.k_proj, sa.v_proj]) + (sa.out_proj.weight.data, sa.out_proj.bias.data) + _mlp_padded(l.mlp)
                        + (l.layer_norm1, l.layer_norm2))
        norms = _Affines([m for m in self.modules() if isinstance(m, _WB) and m.weight.dim() == 1])
        return dict(Fp=(self.config.intermediate_size + 63) // 64 * 64, layers=plan, norms=norms)

    def _padded_tokens(self, S: int) -> int:
        """Rows per batch entry of the token buffers: the fused attention takes S as it is."""
        return S

    def _attention(self, qkv: torch.Tensor, att: torch.Tensor, S: int) -> None:
        d, H = self.config.hidden_size, self.config.num_attention_heads
        fused = ops.attention_hd64 if self._head_dim == 64 else ops.attention_hd72
        fused(qkv[:, :S, :d], qkv[:, :S, d : 2 * d], qkv[:, :S, 2 * d :], att[:, :S], H, self._head_dim ** -0.5)

    def _layers(self, plans: dict, aff: dict, x: torch.Tensor, S: int, act=None) -> None:
        """The pre-LN blocks on the fp32 residual stream x [B,Sp,d] (rows >= S of an entry are padding), in place: LN1 -> q|k|v GEMM
        -> attention -> out-proj + residual -> LN2 -> fc1 -> activation -> fc2 + residual. ``aff``: ``plans["norms"].refresh()``;
        ``act``: a pass over the fc1 output in place, or None for gelu_tanh in fc1's own epilogue."""
        B, Sp, d = x.shape
        dev, eps = x.device, float(self.config.layer_norm_eps)
        x2, x3 = x.view(B * Sp, d), x.view(1, B * Sp, d)
        xn = torch.empty(B, Sp, d, device=dev, dtype=BF16)
        xn2, xn3 = xn.view(B * Sp, d), xn.view(1, B * Sp, d)
        qkv = torch.empty(B, Sp, 3 * d, device=dev, dtype=BF16)
        att = torch.zeros(B, Sp, d, device=dev, dtype=BF16) if Sp != S else torch.empty(B, S, d, device=dev, dtype=BF16)
        qkv2, att2 = qkv.view(B * Sp, 3 * d), att.view(B * Sp, d)
        hid = torch.empty(B * Sp, plans["Fp"], device=dev, dtype=BF16)
        for wqkv, bqkv, wo, bo, w1, b1, w2, b2, ln1, ln2 in plans["layers"]:
            ops.layernorm_modulate(x3, xn3, aff[ln1][1], aff[ln1][0], eps=eps)
            ops.linear(xn2, wqkv, qkv2, bias=bqkv)
            self._attention(qkv, att, S)
            ops.linear(att2, wo, x2, bias=bo, res=x2)
            ops.layernorm_modulate(x3, xn3, aff[ln2][1], aff[ln2][0], eps=eps)
            if act is None:
                ops.linear(xn2, w1, hid, bias=b1, gelu_from=0)
            else:
                ops.linear(xn2, w1, hid, bias=b1)
                act(hid)
            ops.linear(hid, w2, x2, bias=b2, res=x2)


class _AssembledAttention:
    """Mixin over a ``_PreLNStack`` with heads of 64: the attention assembled per (batch, head) by ``_attention_heads`` — tokens padded
    to a multiple of 64 (K of the P·V GEMM), scale 64^-0.5 and the bias of ``_attention_bias``. It is what CLIP text runs (a causal
    mask is a bias), and what tools/bench_image_encoder.py times the fused kernel against."""

    def _padded_tokens(self, S: int) -> int:
        return (S + 63) // 64 * 64

    def _attention_bias(self, S: int, device) -> Optional[torch.Tensor]:
        """f32 [1 or H, S, S], or None."""
        return None

    def _attention(self, qkv: torch.Tensor, att: torch.Tensor, S: int) -> None:
        d, H, Tp = self.config.hidden_size, self.config.num_attention_heads, qkv.shape[1]
        key = (S, Tp, qkv.device)
        if getattr(self, "_assembled_key", None) != key:                          # functions of the shape alone: kept between calls
            self._assembled, self._assembled_key = (_attention_scratch(Tp, qkv.device), self._attention_bias(S, qkv.device)), key
        scratch, bias = self._assembled
        _attention_heads(qkv[..., :d], qkv[..., d : 2 * d], qkv[..., 2 * d :], att, H, bias, 64 ** -0.5, S, Tp, scratch)
