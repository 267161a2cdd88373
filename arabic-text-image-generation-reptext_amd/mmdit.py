"""Shared execution engine of the MMDiT stacks (FLUX transformer and ControlNet tower).

Host side only: it sequences the HIP ops of ops.py over preallocated HBM buffers. Math per SURVEY.md
Appendix A.1 (double-stream block), A.2 (single-stream block), A.5 (embeddings).

HBM layout (B images, T text tokens, N image tokens, S = T+N, d = H·128), all bf16 unless noted:
  x    [B,S,d]    residual stream, TEXT ROWS FIRST (the order attention concatenates them, A.1 step 4)
  xn   [B,S,d]    LayerNorm+modulation output = A operand of the projections
  qkv  [B,S,3d]   double blocks: [q|k|v]; attention output overwrites q in place
  big  [B,S,7d]   single blocks: [k|v|q|mlp]; attention output overwrites q, so proj_out reads the
                  contiguous [attn|mlp] = big[..., 2d:7d] with K = 5d — no concat, no copy
  ffh  [B,S,4d]   double-block feed-forward hidden (image and text rows in one buffer)
  mod  f32        adaLN vectors: [B,6d] per stream (double), [B,3d] (single)
Image and text projections of a double block are issued as ONE grouped GEMM launch each.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from . import native, ops
from .modules import _fuse
from .ops import LinearProblem as P

import os

BF16, F32 = torch.bfloat16, torch.float32
# dtype of the residual stream x. The reference's bf16 run keeps it in bf16 (one rounding per residual add); fp32 (default)
# removes those roundings — measured on MI355X: rel-L2 vs the fp32 oracle 4.8e-3 -> 2.3e-3 on the 2+2-block transformer, for
# +1.9 % time per image (the GEMM epilogue and LayerNorm kernels take either dtype). RT_RESIDUAL_F32=0 selects bf16.
RESIDUAL_F32 = os.environ.get("RT_RESIDUAL_F32", "1") == "1"

# q/k RMSNorm + RoPE inside the QKV GEMM's epilogue (ops.QKRope) instead of a pass of its own over q and k: bf16 path, inner width a
# multiple of 256, no IP-Adapter on the block (rt_ip_attention reads the raw q). Same bits either way; RT_FUSED_QK_ROPE=0 keeps the pass.
FUSED_QK_ROPE = os.environ.get("RT_FUSED_QK_ROPE", "1") == "1"

# The reference's bf16 run rounds the SCALARS that feed the sinusoidal embeddings: PIPE:1025 casts t to the latents' dtype,
# PIPE:1048/1094 divide by 1000 in bf16 and CN:282-284 multiply by 1000 in bf16 again — t = 967.3 enters the embedding as 968,
# guidance 3.5 as 3504. The default here (and in the oracle) is the exact fp32 value, i.e. the fp32 CPU run the parity target
# names; `reference_bf16_scalars(True)` (pipelines: `pipe.reference_bf16_scalars = True`) reproduces the bf16 run's values.
REF_BF16_SCALARS = False


def reference_bf16_scalars(on: bool = True) -> None:
    global REF_BF16_SCALARS
    REF_BF16_SCALARS = bool(on)


def bf16_round_trip_x1000(v: torch.Tensor) -> torch.Tensor:
    """fp32 tensor holding what CN:282-284 computes from a model-scale scalar in a bf16 run: bf16(bf16(v) * 1000)."""
    return (v.to(torch.bfloat16) * 1000).to(torch.float32)


@dataclass
class Proj:
    """One projection of a block: views of its bf16 weight and bias and, where the plan's level quantises it, the e4m3 copy of the
    weight with its per-output-channel scales (None otherwise)."""
    w: torch.Tensor
    b: torch.Tensor
    w8: Optional[torch.Tensor] = None
    ws: Optional[torch.Tensor] = None


@dataclass
class DoublePlan:
    ada_img: Proj
    ada_txt: Proj
    qkv_img: Proj
    qkv_txt: Proj
    out_img: Proj
    out_txt: Proj
    ff1_img: Proj
    ff1_txt: Proj
    ff2_img: Proj
    ff2_txt: Proj
    nq_img: torch.Tensor
    nk_img: torch.Tensor
    nq_txt: torch.Tensor
    nk_txt: torch.Tensor
    # None = bf16; "ln": e4m3 copies of the projections fed by a LayerNorm; "all": also of those whose input is a bf16 activation
    # (attention output, GELU hidden), quantised by a pass; "mx": those read e4m3 + E8M0 block scales written by the producing epilogue
    level: Optional[str] = None
    fp8_attention: bool = False


@dataclass
class SinglePlan:
    ada: Proj
    fused: Proj             # rows: [to_k | to_v | to_q | proj_mlp]
    out: Proj
    nq: torch.Tensor
    nk: torch.Tensor
    level: Optional[str] = None
    fp8_attention: bool = False


def _quantised(pl) -> tuple:
    """The projections of a plan that its level keeps an e4m3 copy of, in the order they are quantised: the LayerNorm-fed ones at
    every level, the activation-fed ones at "all" and "mx"."""
    if isinstance(pl, DoublePlan):
        ln_fed, act_fed = (pl.qkv_img, pl.qkv_txt, pl.ff1_img, pl.ff1_txt), (pl.out_img, pl.out_txt, pl.ff2_img, pl.ff2_txt)
    else:
        ln_fed, act_fed = (pl.fused,), (pl.out,)
    return () if pl.level is None else ln_fed + act_fed if pl.level in ("all", "mx") else ln_fed


def _linear_of(m) -> Proj:
    return Proj(m.weight.data, m.bias.data)


def _set_level(pl, fp8, fp8_attention: bool, d: int):
    """Store the level of a fresh plan (inner width d) once, and quantise the projections it names."""
    pl.level, pl.fp8_attention = "ln" if fp8 is True else (fp8 or None), fp8_attention
    if pl.level == "mx" and d % 256:
        raise ValueError("the 'mx' level needs an inner width that is a multiple of 256")
    for p in _quantised(pl):
        p.w8, p.ws = ops.quantize_rows_fp8(p.w)
    return pl


def plan_double(blk, fp8=False, fp8_attention: bool = False) -> DoublePlan:
    """fp8: False | 'ln' (LayerNorm-fed projections) | 'all' (every projection of the block, per-row scales, one quantise pass per
    bf16 input) | 'mx' (every projection; the non-LayerNorm inputs as e4m3 + block scales written by their producers)."""
    a, lin = blk.attn, _linear_of
    pl = DoublePlan(ada_img=lin(blk.norm1.linear), ada_txt=lin(blk.norm1_context.linear),
                    qkv_img=Proj(*_fuse([a.to_q, a.to_k, a.to_v])), qkv_txt=Proj(*_fuse([a.add_q_proj, a.add_k_proj, a.add_v_proj])),
                    out_img=lin(a.to_out[0]), out_txt=lin(a.to_add_out), ff1_img=lin(blk.ff.net[0].proj), ff1_txt=lin(blk.ff_context.net[0].proj),
                    ff2_img=lin(blk.ff.net[2]), ff2_txt=lin(blk.ff_context.net[2]), nq_img=a.norm_q.weight.data, nk_img=a.norm_k.weight.data,
                    nq_txt=a.norm_added_q.weight.data, nk_txt=a.norm_added_k.weight.data)
    return _set_level(pl, fp8, fp8_attention, pl.out_img.w.shape[1])


def plan_single(blk, fp8=False, fp8_attention: bool = False) -> SinglePlan:
    a = blk.attn
    pl = SinglePlan(_linear_of(blk.norm.linear), Proj(*_fuse([a.to_k, a.to_v, a.to_q, blk.proj_mlp])), _linear_of(blk.proj_out),
                    a.norm_q.weight.data, a.norm_k.weight.data)
    return _set_level(pl, fp8, fp8_attention, pl.out.w.shape[0])


def fp8_copies(pl) -> list:
    """(bf16 weight, e4m3 copy, per-row scales) of every projection of a plan that has an e4m3 copy (enable_fp8_linears)."""
    return [(p.w, p.w8, p.ws) for p in _quantised(pl)]


class Workspace:
    """Preallocated activations for one (B,T,N) shape; reused across blocks, steps and models on the same device."""

    def __init__(self, B: int, T: int, N: int, d: int, device, need_single: bool):
        S = T + N
        self.B, self.T, self.N, self.S, self.d = B, T, N, S, d
        e = lambda *shape, dt=BF16: torch.empty(*shape, device=device, dtype=dt)
        self.x = e(B, S, d, dt=F32 if RESIDUAL_F32 else BF16)
        self.xn = e(B, S, d)
        self.qkv = e(B, S, 3 * d)
        self.ffh = e(B, S, 4 * d)
        self.big = e(B, S, 7 * d) if need_single else None
        self.mod_a = e(B, 6 * d, dt=F32)
        self.mod_b = e(B, 6 * d, dt=F32)
        self.temb = e(B, d, dt=F32)
        self.tmp = e(B, d, dt=F32)
        self._device = device
        self.xn8 = None                            # fp8 path (allocated on first use): e4m3 LayerNorm output + row scales
        self.xs_t = self.xs_i = self.xs_all = None

    def ip_buffer(self) -> torch.Tensor:
        """[B,N,d] bf16: the IP-Adapter term of the running double block (allocated on first use)."""
        if getattr(self, "_ip", None) is None:
            self._ip = torch.empty(self.B, self.N, self.d, device=self._device, dtype=BF16)
        return self._ip

    def ip_buffer_joint(self) -> torch.Tensor:
        """[B,S,d] bf16: the IP-Adapter term of the running single block, all S rows (the InstantX form; allocated on first use)."""
        if getattr(self, "_ip_s", None) is None:
            self._ip_s = torch.empty(self.B, self.S, self.d, device=self._device, dtype=BF16)
        return self._ip_s

    def fp8_buffers(self):
        if self.xn8 is None:
            B, T, N, S, d = self.B, self.T, self.N, self.S, self.d
            self.xn8 = torch.empty(B, S, d, device=self._device, dtype=ops.FP8)
            self.xs_t = torch.empty(B * T, device=self._device, dtype=F32)
            self.xs_i = torch.empty(B * N, device=self._device, dtype=F32)
            self.xs_all = torch.empty(B * S, device=self._device, dtype=F32)
        return self.xn8

    def fp8_attn_buffers(self, H: int):
        """(qk8 [B,S,2·H·128], vt8 flat) of rt_attention_fp8_prep."""
        if getattr(self, "_qk8", None) is None:
            self._qk8 = torch.empty(self.B, self.S, 2 * H * 128, device=self._device, dtype=ops.FP8)
            self._vt8 = torch.empty(int(native.load().rt_attention_fp8_vt_bytes(self.B, self.S, H)), device=self._device, dtype=ops.FP8)
        return self._qk8, self._vt8

    def fp8_wide(self, width: int) -> torch.Tensor:
        """e4m3 staging for quantised bf16 activations: [B,S,width] view of one buffer sized for the widest use (5d)."""
        if getattr(self, "_a8", None) is None or self._a8.shape[2] < width:
            self._a8 = torch.empty(self.B, self.S, max(width, 5 * self.d), device=self._device, dtype=ops.FP8)
        return self._a8[:, :, :width]


    def mx_scales(self) -> "ops.BlockScales":
        """E8M0 block scales of the fp8_wide buffer (one plane per 256 columns, sized for 5d)."""
        if getattr(self, "_a8s", None) is None:
            self._a8s = ops.BlockScales.empty(self.B, self.S, 5 * self.d, self._device)
        return self._a8s


_WS_CACHE = {}
# While a hipGraph of the loop is being captured (pipeline._denoise) every Workspace handed out is also appended here: the graph
# bakes in their device pointers, so its cache entry must OWN them — this cache may evict or replace an entry at any time.
CAPTURE_KEEP: Optional[list] = None


def workspace(B, T, N, d, device, need_single, tag: str = "") -> Workspace:
    """``tag`` separates the buffers of models that may run concurrently on two streams (pipeline: tower vs transformer)."""
    key = (B, T, N, d, str(device), RESIDUAL_F32, tag)
    ws = _WS_CACHE.get(key)
    if ws is None or (need_single and ws.big is None):
        if len(_WS_CACHE) > 6:
            _WS_CACHE.clear()
        ws = Workspace(B, T, N, d, device, need_single)
        _WS_CACHE[key] = ws
    if CAPTURE_KEEP is not None:
        CAPTURE_KEEP.append(ws)
    return ws


def time_text_embed(tte, ws: Workspace, t1000: torch.Tensor, g1000: Optional[torch.Tensor], pooled: torch.Tensor) -> torch.Tensor:
    """temb = MLP(sinusoid(t)) [+ MLP(sinusoid(g))] + MLP(pooled), fp32 [B,d] (A.5; CN:287-291)."""
    def mlp(m, x_f32, accumulate):
        ops.gemv(x_f32, m.linear_1.weight.data, m.linear_1.bias.data, ws.tmp, silu_out=True)
        ops.gemv(ws.tmp, m.linear_2.weight.data, m.linear_2.bias.data, ws.temb, accumulate=accumulate)

    mlp(tte.timestep_embedder, ops.timestep_embedding(t1000, 256), False)
    if g1000 is not None:
        mlp(tte.guidance_embedder, ops.timestep_embedding(g1000, 256), True)
    pooled_f32 = pooled if pooled.dtype == F32 else ops.to_f32(pooled)
    mlp(tte.text_embedder, pooled_f32.contiguous(), True)
    return ws.temb


def time_text_embed_all(tte, t1000_all: torch.Tensor, g1000: Optional[torch.Tensor], pooled: torch.Tensor, B: int) -> torch.Tensor:
    """time_text_embed for every step of a schedule: fp32 [n·B, d], row i·B + b = step i, image b. t1000_all [n·B] in that order;
    g1000 [B] / pooled [B,P] are the same at every step, so their MLPs run once and only the timestep MLP runs per step — all steps
    in one batch of GEMV rows (a row's result does not depend on the rows it is launched with). Each row is (t + g) + p in fp32, the
    order in which time_text_embed accumulates: the same bits."""
    dev = pooled.device
    d = tte.timestep_embedder.linear_2.weight.shape[0]

    def mlp(m, x_f32):
        h = torch.empty(x_f32.shape[0], m.linear_1.weight.shape[0], device=dev, dtype=F32)
        y = torch.empty(x_f32.shape[0], d, device=dev, dtype=F32)
        ops.gemv(x_f32, m.linear_1.weight.data, m.linear_1.bias.data, h, silu_out=True)
        ops.gemv(h, m.linear_2.weight.data, m.linear_2.bias.data, y)
        return y

    temb_all = mlp(tte.timestep_embedder, ops.timestep_embedding(t1000_all, 256))
    pooled_f32 = pooled if pooled.dtype == F32 else ops.to_f32(pooled)
    p = mlp(tte.text_embedder, pooled_f32.contiguous())
    if g1000 is not None:
        ops.add_rows_(temb_all, mlp(tte.guidance_embedder, ops.timestep_embedding(g1000, 256)), p)
    else:
        ops.add_rows_(temb_all, p)
    return temb_all


@dataclass
class StepMods:
    """adaLN vectors of one denoising step, per block: fp32 row-slices of a ModulationTable."""

    double: List[tuple]                  # (image [B,6d], text [B,6d])
    single: List[torch.Tensor]           # [B,3d]
    out: Optional[torch.Tensor]          # [B,2d] (norm_out), transformer only


class ModulationTable:
    """All adaLN projections `linear(silu(temb))` (A.1 step 1, A.2, A.3) of a model for EVERY step of a schedule at once.

    temb depends only on (timestep, guidance, pooled text) — all known before the loop (PIPE:960-967,1025-1032) — so the
    63 per-step weight-streaming GEMVs (6.4 GB of adaLN weights per step) become one M = steps·B GEMM per block, issued
    once per image: the weights are streamed twice (hi + lo pass) instead of `steps` times. The two-term bf16 split of
    silu(temb) keeps fp32-activation accuracy on the bf16 MFMA path."""

    def __init__(self, temb_all: torch.Tensor, n_steps: int, B: int, doubles, singles, out_lin=None):
        self.n, self.B = n_steps, B
        hi, lo = ops.silu_split(temb_all, apply_silu=True)
        dev = temb_all.device
        M = temb_all.shape[0]

        def out_buf(w):
            return torch.empty(M, w.shape[0], device=dev, dtype=F32)

        self.double, self.single, self.out = [], [], None
        # M <= 32 rows with K % 256 == 0 (28 steps at batch 1): the skinny kernel streams each weight once for both terms, one launch
        # per block; otherwise the general GEMM, two launches (hi, then lo accumulated onto it). The two give the same bits.
        skinny = M <= 32 and temb_all.shape[1] % 256 == 0 and all(w.shape[0] % 16 == 0 for w in self._widths(doubles, singles, out_lin))

        def table(problems):
            if skinny:
                ops.linear_skinny(hi, lo, problems)
            else:
                ops.linear_grouped([P(hi, w, o, bias=b) for w, b, o in problems])
                ops.linear_grouped([P(lo, w, o, res=o) for w, b, o in problems])

        for pl in doubles:
            oi, ot = out_buf(pl.ada_img.w), out_buf(pl.ada_txt.w)
            table([(pl.ada_img.w, pl.ada_img.b, oi), (pl.ada_txt.w, pl.ada_txt.b, ot)])
            self.double.append((oi, ot))
        for pl in singles:
            o = out_buf(pl.ada.w)
            table([(pl.ada.w, pl.ada.b, o)])
            self.single.append(o)
        if out_lin is not None:
            o = out_buf(out_lin.weight.data)
            table([(out_lin.weight.data, out_lin.bias.data, o)])
            self.out = o

    @staticmethod
    def _widths(doubles, singles, out_lin):
        return [w for pl in doubles for w in (pl.ada_img.w, pl.ada_txt.w)] + [pl.ada.w for pl in singles] + ([out_lin.weight.data] if out_lin is not None else [])

    def step(self, i: int, rows: Optional[slice] = None) -> StepMods:
        """The rows of step i, or with ``rows`` a slice of them (the positive half of a true-CFG table is the second half). Views."""
        r = slice(i * self.B, (i + 1) * self.B) if rows is None else slice(i * self.B + rows.start, i * self.B + rows.stop)
        return StepMods([(a[r], b[r]) for a, b in self.double], [s[r] for s in self.single], None if self.out is None else self.out[r])


def _ch(m: torch.Tensor, i: int, d: int) -> torch.Tensor:
    """Chunk i of a stream's adaLN vectors. Double block: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp; single
    block: shift, scale, gate."""
    return m[:, i * d : (i + 1) * d]


def _row_scales(ws: Workspace, r: slice) -> torch.Tensor:
    """fp32 per-row scales of the e4m3 rows r of every image: one contiguous [B·rows] buffer for each stream (all rows, text, image)."""
    ws.fp8_buffers()
    return ws.xs_all if (r.start, r.stop) == (0, ws.S) else ws.xs_t if r.stop == ws.T else ws.xs_i


def _ln_linear(ws: Workspace, level: Optional[str], c: int, out: torch.Tensor, streams, ropes=None, mx_out=None) -> bool:
    """The projections fed by a LayerNorm. For one or two row streams of ws.x — ``streams`` = (rows, adaLN vectors, Proj, epilogue
    arguments) each, the image stream first — LayerNorm + modulation with chunks c (shift) and c + 1 (scale), then the ONE grouped GEMM
    that reads the result into the same rows of ``out``.
      bf16          one LayerNorm launch (the pair kernel for two streams) into ws.xn, the bf16 weights; ``ropes`` (a QKRope per stream)
                    ride this GEMM's epilogue, which no e4m3 GEMM has: returns whether they were applied
      e4m3 levels   one quantising LayerNorm per stream into e4m3 rows + per-row scales, the e4m3 weights
      "mx"          also, with ``mx_out`` = (width, col0, first): columns first.. of the result (the GELU hidden) leave the epilogue as
                    e4m3 + block scales, columns col0.. of the width-wide operand of the projection that reads them (out does not get them)"""
    d = ws.d
    if level is None:
        ln = [(ws.x[:, r], ws.xn[:, r], _ch(m, c, d), _ch(m, c + 1, d)) for r, m, _, _ in streams]
        if len(ln) == 2:
            ops.layernorm_modulate_pair(*ln[0], *ln[1])
        else:
            ops.layernorm_modulate(*ln[0])
        ops.linear_grouped([P(ws.xn[:, r], p.w, out[:, r], bias=p.b, rope=ropes[i] if ropes else None, **kw)
                            for i, (r, _, p, kw) in enumerate(streams)])
        return ropes is not None
    xn8, problems = ws.fp8_buffers(), []
    for r, m, p, kw in streams:
        xs = _row_scales(ws, r)
        ops.layernorm_modulate_fp8(ws.x[:, r], xn8[:, r], xs, _ch(m, c, d), _ch(m, c + 1, d))
        if level == "mx" and mx_out is not None:
            width, col0, first = mx_out
            kw = dict(kw, out8=ws.fp8_wide(width)[:, r, col0:], out8_scales=ws.mx_scales().rows(r.start).cols(col0), out8_from=first)
        problems.append(P(xn8[:, r], p.w8, out[:, r], bias=p.b, a_scale=xs, w_scale=p.ws, **kw))
    ops.linear_grouped(problems)
    return False


def _act_linear(ws: Workspace, level: Optional[str], src: torch.Tensor, out: torch.Tensor, streams, fresh: int) -> None:
    """The projections of a bf16 activation ``src`` [B,S,K] (attention output, GELU hidden): ONE grouped GEMM from the rows of src into
    the same rows of ``out``; ``streams`` = (rows, Proj, epilogue arguments) each, the image stream first.
      bf16, "ln"    the bf16 weights on src itself
      "all"         one per-row quantise pass per stream into the e4m3 staging buffer, then the e4m3 weights
      "mx"          the staging buffer with its block scales; the producer's epilogue has written it, except the first ``fresh``
                    columns, which exist in src only and take one block-quantise pass (all rows)"""
    if level not in ("all", "mx"):
        ops.linear_grouped([P(src[:, r], p.w, out[:, r], bias=p.b, **kw) for r, p, kw in streams])
        return
    a8, problems = ws.fp8_wide(src.shape[2]), []
    if level == "mx" and fresh:
        ops.quantize_mx_fp8_into(src[..., :fresh], a8[..., :fresh], ws.mx_scales())
    for r, p, kw in streams:
        if level == "mx":
            scale = dict(a_bscale=ws.mx_scales().rows(r.start))
        else:
            scale = dict(a_scale=_row_scales(ws, r))
            ops.quantize_rows_fp8_into(src[:, r], a8[:, r], scale["a_scale"])
        problems.append(P(a8[:, r], p.w8, out[:, r], bias=p.b, w_scale=p.ws, **scale, **kw))
    ops.linear_grouped(problems)


def _double_front(pl: DoublePlan, ws: Workspace, temb, cos, sin, mods: Optional[tuple], rope: bool) -> tuple:
    """Steps 1-3 of a double block, shared by run_double and its windowed mode: (image, text adaLN vectors, whether the QKV GEMM applied
    q/k RMSNorm + RoPE). The unfused norm + RoPE pass is the caller's: the IP-Adapter launches need the raw query first."""
    T, d = ws.T, ws.d
    # 1. adaLN-Zero vectors
    if mods is not None:
        mi, mt = mods
    else:
        mi, mt = ws.mod_a, ws.mod_b
        ops.gemv(temb, pl.ada_img.w, pl.ada_img.b, mi, silu_in=True)
        ops.gemv(temb, pl.ada_txt.w, pl.ada_txt.b, mt, silu_in=True)
    # 2. norm + modulate, 3. q,k,v projections of both streams, one launch
    ropes = (ops.QKRope(0, d, d, pl.nq_img, pl.nk_img, cos, sin, pos0=T), ops.QKRope(0, d, d, pl.nq_txt, pl.nk_txt, cos, sin, pos0=0))
    fused = _ln_linear(ws, pl.level, 0, ws.qkv, [(slice(T, ws.S), mi, pl.qkv_img, {}), (slice(0, T), mt, pl.qkv_txt, {})],
                       ropes=ropes if rope and FUSED_QK_ROPE and ops.QKRope.covers(d) else None)
    return mi, mt, fused


def _ip_terms(ip) -> list:
    """``ip`` of a block as a list of (K, V, scale, row weights): a plain (K, V, scale) tuple is one term without weights."""
    if ip is None:
        return []
    if isinstance(ip[0], torch.Tensor):
        return [(ip[0], ip[1], ip[2], None)]
    return [tuple(t) + (None,) * (4 - len(t)) for t in ip]


def run_double(pl: DoublePlan, ws: Workspace, temb: torch.Tensor, cos, sin, H: int, inject: Optional[torch.Tensor] = None,
               mods: Optional[tuple] = None, ip: Optional[tuple] = None, ip_inside: bool = False,
               window: Optional[tuple] = None, groups: Optional["ops.KeyGroups"] = None, key_bias: Optional[torch.Tensor] = None,
               self_key: bool = False) -> None:
    """One FluxTransformerBlock on ws.x in place (A.1). ``inject`` [B,N,d] bf16 is added to the image rows after the
    block (A.3 ControlNet residual), fused into the last GEMM's epilogue. ``mods`` = precomputed (image, text) adaLN
    vectors for this step (ModulationTable); computed here from ``temb`` when absent. ``ip`` = (K, V, scale) of an IP-Adapter
    (ip_adapter.py): scale · softmax(q Kᵀ/√128) V from the image query after norm_q and before RoPE, added to the image rows after the
    feed-forward residual. ``ip_inside`` = the InstantX form of the same tuple: gate_msa · scale · softmax(q Kᵀ/√128) V, K used as given,
    accumulated straight onto the residual image rows by ONE launch placed where the raw query exists (before attention); the later
    x += gate_msa · to_out(attn) epilogue adds onto it, so h <- h + gate_msa · (to_out(attn) + scale · ip) up to the order of two
    fp32 additions. With ``ip=None`` the launch sequence is unchanged. ``window`` = (r0, r1): the caller reads nothing of this block
    but image rows [r0, r1) of the stream (the last evaluated block of a ControlNet tower under a regional mask, whose only reader is
    its zero-linear): keys and values are still computed for all S rows, but attention runs only for the items of its launch that hold a
    window query (same cut, same bits), the image
    out / LayerNorm / ff1 / ff2 on the window's rows only, and nothing of the text stream after the QKV projection. The other rows of
    ws.x are left as they were before the block. bf16 projections and attention without ``ip`` / ``inject`` only. ``groups`` (an
    ops.KeyGroups over the S joint rows): the region-masked joint attention of per-line prompts, bf16 attention only; nothing else of the
    block changes. ``ip`` may also be a sequence of (K, V, scale, row_weights) terms, regional image prompts (ip_adapter.py): the
    first takes the slot the single term takes, each further one accumulates into the same place with one more rounding, in order;
    ``row_weights`` (fp32 [B or 1, N], or None) is the per-row weight of ops.ip_attention_gated. ``key_bias`` (only with ``groups``):
    ops.attention's bias per key group or class, the biased launch in place of the grouped or keyed one. ``self_key`` (only with
    ``groups`` as an ops.KeyClasses): ops.attention's self rule, row i also sees key i (perturbed-attention guidance)."""
    T, d = ws.T, ws.d
    terms = _ip_terms(ip)
    ip = terms or None
    if key_bias is not None and groups is None:
        raise ValueError("run_double: key_bias needs key groups")
    if self_key and groups is None:
        raise ValueError("run_double: self_key needs key groups")
    akw = dict(key_bias=key_bias) if key_bias is not None else {}
    if self_key:
        akw["self_key"] = True
    if groups is not None and (pl.fp8_attention or window is not None):
        raise ValueError("run_double: key groups need the bf16 attention kernel and the whole block (no e4m3 attention, no window)")
    if window is not None:
        if ip is not None or inject is not None or pl.level is not None or pl.fp8_attention:
            raise ValueError("run_double: the windowed mode is the bf16 path without ip / inject")
        return _run_double_window(pl, ws, temb, cos, sin, H, mods, int(window[0]), int(window[1]))
    txt, img = slice(0, T), slice(T, ws.S)
    x_t, x_i = ws.x[:, txt], ws.x[:, img]
    mi, mt, fused_rope = _double_front(pl, ws, temb, cos, sin, mods, rope=ip is None and not pl.fp8_attention)
    q, k, v = ws.qkv[..., :d], ws.qkv[..., d : 2 * d], ws.qkv[..., 2 * d :]
    if ip is not None and ip_inside:
        for K, V, s, w in terms:
            ops.ip_attention_gated(q[:, T:], pl.nq_img, K, V, x_i, H, ip_scale=s, gate=_ch(mi, 2, d), accumulate=True, row_weights=w)
        ip = None
    if ip is not None:
        # the raw image query is only here: qk_rmsnorm_rope works in place and the attention output overwrites q
        ip_out = ws.ip_buffer()
        for j, (K, V, s, w) in enumerate(terms):
            ops.ip_attention(q[:, T:], pl.nq_img, K, V, ip_out, H, ip_scale=s, accumulate=j > 0, row_weights=w)
        if inject is None:
            inject, ip = ip_out, None                # no ControlNet sample: the term rides the add2 slot of the ff2 epilogue
    attn_mx = pl.fp8_attention and pl.level == "mx"           # the attention kernel is the producer of the out-projections' operand
    if pl.fp8_attention:
        # 4.-6. RMSNorm(q,k) + RoPE -> e4m3 q|k and permuted Vᵀ, e4m3 joint attention; output over q ("mx": straight into the
        # out-projections' e4m3 operand with its block scales)
        qk8, vt8 = ws.fp8_attn_buffers(H)
        ops.attention_fp8_prep(ws.qkv, 0, d, 2 * d, H, T, pl.nq_txt, pl.nk_txt, pl.nq_img, pl.nk_img, cos, sin, qk8, vt8)
        if attn_mx:
            ops.attention_fp8_mx(qk8, vt8, ws.fp8_wide(d), ws.mx_scales(), H)
        else:
            ops.attention_fp8(qk8, vt8, q, H)
    else:
        # 4.-5. RMSNorm(q,k) + RoPE in place; 6. joint attention; output over q
        if not fused_rope:
            ops.qk_rmsnorm_rope(ws.qkv, 0, d, H, T, pl.nq_txt, pl.nk_txt, pl.nq_img, pl.nk_img, cos, sin)
        ops.attention(q, k, v, q, H, groups=groups, **akw)
    # 7./8. x += gate_msa * out_proj(attn)
    _act_linear(ws, pl.level, q, ws.x, [(img, pl.out_img, dict(gate=_ch(mi, 2, d), res=x_i)),
                                        (txt, pl.out_txt, dict(gate=_ch(mt, 2, d), res=x_t))], fresh=0 if attn_mx else d)
    # "mx": the GELU hidden leaves the epilogue as e4m3 + block scales (ffh is not written)
    _ln_linear(ws, pl.level, 3, ws.ffh, [(img, mi, pl.ff1_img, dict(gelu_from=0)), (txt, mt, pl.ff1_txt, dict(gelu_from=0))], mx_out=(4 * d, 0, 0))
    _act_linear(ws, pl.level, ws.ffh, ws.x, [(img, pl.ff2_img, dict(gate=_ch(mi, 5, d), res=x_i, add2=inject)),
                                             (txt, pl.ff2_txt, dict(gate=_ch(mt, 5, d), res=x_t))], fresh=0)
    if ip is not None:                               # the add2 slot holds the ControlNet sample: one accumulate pass per image
        for b in range(ws.B):
            ops.masked_accumulate_(ws.x[b, T:].unsqueeze(0), ip_out[b : b + 1], None, 1.0, True)


def _run_double_window(pl: DoublePlan, ws: Workspace, temb, cos, sin, H: int, mods: Optional[tuple], r0: int, r1: int) -> None:
    """run_double's windowed mode (see there). The front is run_double's own: every row's k and v are needed. The q columns are
    still projected for all rows and both streams: the fused q/k epilogue of the QKV GEMM describes a group that holds both q and k, and
    restricting q to the window (one tile round of three at the headline shape) is not built."""
    T, d = ws.T, ws.d
    if not (0 <= r0 < r1 <= ws.N):
        raise ValueError(f"window [{r0}, {r1}) is not inside the {ws.N} image rows")
    mi, _, fused_rope = _double_front(pl, ws, temb, cos, sin, mods, rope=True)
    if not fused_rope:
        ops.qk_rmsnorm_rope(ws.qkv, 0, d, H, T, pl.nq_txt, pl.nk_txt, pl.nq_img, pl.nk_img, cos, sin)
    q, k, v = ws.qkv[..., :d], ws.qkv[..., d : 2 * d], ws.qkv[..., 2 * d :]
    # the full launch's own cut, with only the items that hold a window row at work: the window's rows keep the bits of the full path
    ops.attention(q, k, v, q, H, rows=(T + r0, T + r1))
    win = slice(T + r0, T + r1)                               # the window's attention output lies over its queries
    xw = ws.x[:, win]
    _act_linear(ws, pl.level, q, ws.x, [(win, pl.out_img, dict(gate=_ch(mi, 2, d), res=xw))], fresh=d)
    _ln_linear(ws, pl.level, 3, ws.ffh, [(win, mi, pl.ff1_img, dict(gelu_from=0))])
    _act_linear(ws, pl.level, ws.ffh, ws.x, [(win, pl.ff2_img, dict(gate=_ch(mi, 5, d), res=xw))], fresh=0)


def run_single(pl: SinglePlan, ws: Workspace, temb: torch.Tensor, cos, sin, H: int, inject: Optional[torch.Tensor] = None,
               mods: Optional[torch.Tensor] = None, ip: Optional[tuple] = None, groups: Optional["ops.KeyGroups"] = None,
               key_bias: Optional[torch.Tensor] = None, self_key: bool = False) -> None:
    """One FluxSingleTransformerBlock on ws.x in place (A.2). ``ip`` = (K, V, scale) of an InstantX IP-Adapter (ip_adapter.py):
    scale · softmax(q Kᵀ/√128) V from the query of ALL S rows after norm_q and before RoPE, added to the attention output before
    proj_out. The raw q only exists between the fused GEMM and norm + RoPE and attention overwrites it, so the term waits in a bf16
    [B,S,d] buffer and one strided add puts it over q's columns after attention. Wherever the attention output would skip bf16 (the
    "mx" level with e4m3 attention) such a block takes the bf16-output attention call and the quantise pass instead. With ``ip=None``
    the launch sequence is unchanged. ``groups``, ``key_bias``, ``self_key``: as in run_double. ``ip`` may also be a sequence of (K, V, scale, row_weights)
    terms as in run_double, with ``row_weights`` over all S rows: the first writes the buffer, the others accumulate into it."""
    T, d = ws.T, ws.d
    terms = _ip_terms(ip)
    ip = terms or None
    if key_bias is not None and groups is None:
        raise ValueError("run_single: key_bias needs key groups")
    if self_key and groups is None:
        raise ValueError("run_single: self_key needs key groups")
    akw = dict(key_bias=key_bias) if key_bias is not None else {}
    if self_key:
        akw["self_key"] = True
    if groups is not None and pl.fp8_attention:
        raise ValueError("run_single: key groups need the bf16 attention kernel (the e4m3 attention has no mask)")
    if mods is not None:
        m = mods
    else:
        m = ws.mod_a[:, : 3 * d]
        ops.gemv(temb, pl.ada.w, pl.ada.b, m, silu_in=True)                   # shift, scale, gate
    big, rows = ws.big, slice(0, ws.S)
    # [k|v|q|gelu(mlp)]. "mx": the gelu(mlp) columns leave the epilogue as columns d.. of proj_out's e4m3 operand [attn|mlp], with their block scales
    rope = FUSED_QK_ROPE and ip is None and not pl.fp8_attention and ops.QKRope.covers(d)
    fused_rope = _ln_linear(ws, pl.level, 0, big, [(rows, m, pl.fused, dict(gelu_from=3 * d))], mx_out=(5 * d, d, 3 * d),
                            ropes=(ops.QKRope(2 * d, 0, d, pl.nq, pl.nk, cos, sin),) if rope else None)
    q = big[..., 2 * d : 3 * d]
    if ip is not None:
        ip_out = ws.ip_buffer_joint()
        for j, (K, V, s, w) in enumerate(terms):
            ops.ip_attention_gated(q, pl.nq, K, V, ip_out, H, ip_scale=s, accumulate=j > 0, row_weights=w)
    attn_mx = pl.fp8_attention and pl.level == "mx" and ip is None
    if pl.fp8_attention:
        qk8, vt8 = ws.fp8_attn_buffers(H)
        ops.attention_fp8_prep(big, 2 * d, 0, d, H, 0, None, None, pl.nq, pl.nk, cos, sin, qk8, vt8)
        if attn_mx:
            ops.attention_fp8_mx(qk8, vt8, ws.fp8_wide(5 * d)[..., :d], ws.mx_scales(), H)
        else:
            ops.attention_fp8(qk8, vt8, q, H)
    else:
        if not fused_rope:
            ops.qk_rmsnorm_rope(big, 2 * d, 0, H, 0, None, None, pl.nq, pl.nk, cos, sin)
        ops.attention(q, big[..., :d], big[..., d : 2 * d], q, H, groups=groups, **akw)
    if ip is not None:
        ops.add_bf16_(q, ip_out)
    _act_linear(ws, pl.level, big[..., 2 * d :], ws.x, [(rows, pl.out, dict(gate=_ch(m, 2, d), res=ws.x))], fresh=0 if attn_mx else d)
    if inject is not None:                                                       # A.3: image tokens only
        for b in range(ws.B):   # image rows of one batch entry are contiguous; one call per image
            ops.masked_accumulate_(ws.x[b, T:].unsqueeze(0), inject[b : b + 1].contiguous(), None, 1.0, True)


def image_rows_bf16(ws: Workspace, rows: Optional[tuple] = None) -> torch.Tensor:
    """bf16 view/copy of the image rows of the residual stream, as a GEMM A operand (ControlNet zero-linears, CN:384-392).
    With a bf16 stream this is the stream itself; with an fp32 stream the rows are cast into the (free) xn buffer. ``rows`` = (r0, r1):
    only those image rows (cast and returned)."""
    T = ws.T
    r0, r1 = (0, ws.N) if rows is None else (int(rows[0]), int(rows[1]))
    if ws.x.dtype == BF16:
        return ws.x[:, T + r0 : T + r1]
    for b in range(ws.B):
        src, dst = ws.x[b, T + r0 : T + r1], ws.xn[b, T + r0 : T + r1]
        native.call("rt_cast_f32_to_bf16", ops._dev(src, "x", F32), ops._dev(dst, "xn", BF16), src.numel(), ops._stream())
    return ws.xn[:, T + r0 : T + r1]
