"""Tensor-level wrappers over the C ABI (native.py). PyTorch supplies device memory and the stream only.

Every function validates device/dtype/contiguity, then enqueues ONE native call on torch's current HIP
stream. Nothing here computes with torch ops; a CPU tensor is an error, not a fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import torch

from . import native

BF16 = torch.bfloat16
F32 = torch.float32
FP8 = torch.float8_e4m3fn        # OCP e4m3 (what gfx950's conversion and MFMA instructions use)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str, dtype=None) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the HIP path has no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def _opt(t: Optional[torch.Tensor], name: str, dtype=None) -> Optional[int]:
    return None if t is None else _dev(t, name, dtype)


def _rowmajor2d(t: torch.Tensor, name: str):
    """Return (rows, cols, ld) for a 2-D view whose last dim is unit-stride."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


def _batched(t: torch.Tensor, name: str):
    """(batch, rows, cols, ld, batch_stride) of a [R,C] or [B,R,C] view with unit inner stride."""
    if t.dim() == 2:
        r, c, ld = _rowmajor2d(t, name)
        return 1, r, c, ld, 0
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError(f"{name}: need [R,C] or [B,R,C] with unit inner stride, got {tuple(t.shape)} / {t.stride()}")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1), t.stride(0)


def _rows3(t: torch.Tensor, name: str, width: Optional[int] = None, shape=None):
    """(B, R, D, ld, batch_stride) of a [B,R,D] view with unit inner stride; D == width and t.shape == shape where given."""
    if t.dim() != 3 or t.stride(2) != 1 or (width is not None and t.shape[2] != width) or (shape is not None and t.shape != shape):
        want = ",".join(map(str, shape)) if shape is not None else f"B,R,{'D' if width is None else width}"
        raise ValueError(f"{name}: need a [{want}] view with unit inner stride, got {tuple(t.shape)} / {t.stride()}")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1), t.stride(0)


def _modulation(shift: Optional[torch.Tensor], scale: Optional[torch.Tensor], B: int, D: int) -> int:
    """mod_ld of a LayerNorm's shift/scale pair: [B,D] views with unit inner stride and one row stride; 0 without a scale."""
    if scale is None:
        return 0
    if scale.shape != (B, D) or shift.shape != (B, D) or scale.stride(1) != 1 or shift.stride(1) != 1 or scale.stride(0) != shift.stride(0):
        raise ValueError("shift/scale must be [B,D] views with equal row stride")
    return scale.stride(0)


def _is_f32(x: torch.Tensor, name: str = "x") -> int:
    """The x_f32 flag of an operand that may be bf16 or f32."""
    if x.dtype not in (BF16, F32):
        raise TypeError(f"{name} must be bf16 or f32")
    return int(x.dtype == F32)


@dataclass
class BlockScales:
    """E8M0 block scales of an e4m3 activation tensor [B, R, D] (one byte per 32 consecutive elements of a row) in rt_gemm_group's
    layout: ``t`` uint8 [ceil(D/1024), B*Rp/64, 8, 16, 4, 4] = [plane of 1024 columns][64-row chunk][K-tile of 128 columns][row & 15]
    [32-block of the K-tile][row >> 4 & 3], Rp = R rounded up to 64 (rows between batch entries). ``rows(r0)`` / ``cols(k0)``
    address a sub-view of the e4m3 tensor (rows r0.. of every batch entry, r0 % 64 == 0; columns k0.., k0 % 128 == 0: a GEMM's A
    operand must start at column 0, producers may write at any k0)."""

    t: torch.Tensor
    R: int                  # rows between batch entries (multiple of 64)
    row0: int = 0
    k0: int = 0

    @staticmethod
    def empty(B: int, R: int, D: int, device) -> "BlockScales":
        if D % 128:
            raise ValueError("block-scaled rows need D % 128 == 0")
        Rp = (R + 63) // 64 * 64
        return BlockScales(torch.empty((D + 1023) // 1024, B * Rp // 64, 8, 16, 4, 4, device=device, dtype=torch.uint8), Rp)

    @property
    def plane(self) -> int:
        return self.t.stride(0)

    def rows(self, r0: int) -> "BlockScales":
        if r0 % 64:
            raise ValueError("row offset of block scales must be a multiple of 64 (text length T % 64 == 0)")
        return BlockScales(self.t, self.R, self.row0 + r0, self.k0)

    def cols(self, k0: int) -> "BlockScales":
        if k0 % 128:
            raise ValueError("column offset of block scales must be a multiple of 128")
        return BlockScales(self.t, self.R, self.row0, self.k0 + k0)

    def ptr(self) -> int:
        """Device address of the view's row origin (the column origin k0 travels separately)."""
        if not self.t.is_cuda or self.t.dtype != torch.uint8 or not self.t.is_contiguous():
            raise TypeError("block scales must be a contiguous uint8 tensor on the GPU")
        return self.t.data_ptr() + (self.row0 // 64) * 2048

    def columns_left(self) -> int:
        return self.t.shape[0] * 1024 - self.k0

    def _rm(self) -> torch.Tensor:
        """[rows_total, planes*32] row-major view-copy of the whole tensor (row = chunk*64 + i*16 + l15; col = plane*32 + ktile*4 + j)."""
        P = self.t.shape[0]
        return self.t.permute(1, 5, 3, 0, 2, 4).reshape(-1, P * 32)

    def rowmajor(self, B: int, R: int, D: int) -> torch.Tensor:
        """uint8 [B, R, D/32] copy of the view's scale bytes in plain row-major order (tests and tools)."""
        return self._rm().view(-1, self.R, self.t.shape[0] * 32)[:B, self.row0 : self.row0 + R, self.k0 // 32 : (self.k0 + D) // 32].contiguous()

    def set_rowmajor(self, sb: torch.Tensor) -> None:
        """Inverse of rowmajor(): write scale bytes given as uint8 [B, R, D/32] into the view (tests and tools)."""
        B, R, nb = sb.shape
        P = self.t.shape[0]
        full = self._rm().view(-1, self.R, P * 32).clone()
        full[:B, self.row0 : self.row0 + R, self.k0 // 32 : self.k0 // 32 + nb] = sb.to(full.device)
        C = self.t.shape[1]
        self.t.copy_(full.view(C, 4, 16, P, 8, 4).permute(3, 0, 4, 2, 5, 1))


@dataclass
class QKRope:
    """Fused q/k RMSNorm + RoPE of a bf16 LinearProblem (rt_gemm_group::rope_*): columns [q0, q0+width) and [k0, k0+width) of out
    leave the GEMM as qk_rmsnorm_rope would rewrite them. wq / wk bf16 [128] = the norm weights of this problem's rows; cos / sin f32
    [positions,128]; pos0 = table row of the problem's row 0 in a batch entry. q0, k0, width % 256 == 0."""

    q0: int
    k0: int
    width: int
    wq: torch.Tensor
    wk: torch.Tensor
    cos: torch.Tensor
    sin: torch.Tensor
    pos0: int = 0
    eps: float = 1e-6

    @staticmethod
    def covers(width: int) -> bool:
        return width % 256 == 0


@dataclass
class LinearProblem:
    """One group of rt_gemm_bf16: out = epilogue(a @ w.T + bias).

    a [M,K] or [B,M,K] bf16 views (unit inner stride); w [N,K] bf16; out [.., M, N] bf16|f32.
    gate f32: [B,N] view (one vector per batch) — or, for 2-D problems whose rows are batch-major,
    [M/rows_per_batch, N] with rows_per_batch set. res same dtype/shape as out (may alias it);
    add2 bf16 same shape; rowscale f32 [rows_per_batch or M] shared by the batch, or [B, rows] (one vector per batch entry)."""

    a: torch.Tensor
    w: torch.Tensor
    out: torch.Tensor
    bias: Optional[torch.Tensor] = None
    gate: Optional[torch.Tensor] = None
    res: Optional[torch.Tensor] = None
    add2: Optional[torch.Tensor] = None
    rowscale: Optional[torch.Tensor] = None
    rows_per_batch: int = 0
    gelu_from: Optional[int] = None
    alpha: float = 1.0
    # fp8 problems (rt_gemm_fp8): a and w are float8_e4m3fn, a_scale f32 [B*M] (one per activation row), w_scale f32 [N]
    a_scale: Optional[torch.Tensor] = None
    w_scale: Optional[torch.Tensor] = None
    # MX block scales (fp8 problems): a_bscale = the block scales of a; out8 / out8_scales = e4m3 + block-scale output for the
    # columns >= out8_from (those columns are then not written to out): the next projection's operand, no pass in between
    a_bscale: Optional[BlockScales] = None
    out8: Optional[torch.Tensor] = None
    out8_scales: Optional[BlockScales] = None
    out8_from: int = 0
    rope: Optional[QKRope] = None       # bf16 problems: fused q/k RMSNorm + RoPE

    @property
    def is_fp8(self) -> bool:
        return self.a.dtype == FP8

    def to_group(self) -> native.GemmGroup:
        Bt, M, K, lda, sA = _batched(self.a, "a")
        N, Kw, ldw = _rowmajor2d(self.w, "w")
        Bo, Mo, No, ldc, sC = _batched(self.out, "out")
        if Kw != K or Mo != M or No != N or Bo != Bt:
            raise ValueError(f"linear shapes mismatch: a{tuple(self.a.shape)} w{tuple(self.w.shape)} out{tuple(self.out.shape)}")
        g = native.GemmGroup()
        op_dtype = FP8 if self.is_fp8 else BF16
        g.A = _dev(self.a, "a", op_dtype)
        g.W = _dev(self.w, "w", op_dtype)
        if self.is_fp8:
            if self.a_scale is not None:
                if self.a_scale.numel() != Bt * M or not self.a_scale.is_contiguous():
                    raise ValueError("a_scale must be contiguous with batch*M elements")
                g.a_scale = _dev(self.a_scale, "a_scale", F32)
            if self.w_scale is not None:
                if self.w_scale.numel() != N or not self.w_scale.is_contiguous():
                    raise ValueError("w_scale must be contiguous with N elements")
                g.w_scale = _dev(self.w_scale, "w_scale", F32)
            if self.a_bscale is not None:
                if self.a_bscale.k0 != 0 or self.a_bscale.columns_left() < K:
                    raise ValueError("block-scaled a: the operand starts at column 0 of its scale tensor, which must cover K")
                g.a_bscale, g.a_bscale_plane, g.a_bscale_rows = self.a_bscale.ptr(), self.a_bscale.plane, self.a_bscale.R
            if self.out8 is not None:
                B8, M8, N8, ld8, s8 = _batched(self.out8, "out8")
                if self.out8_scales is None or (B8, M8) != (Bt, M) or N8 != N - self.out8_from or self.out8_scales.columns_left() < N8:
                    raise ValueError("out8 must be [.., M, N - out8_from] e4m3 with its block scales")
                g.c8, g.c_bscale = _dev(self.out8, "out8", FP8), self.out8_scales.ptr()
                g.ldc8, g.stride_c8, g.c_bscale_plane, g.c_bscale_rows, g.c8_from = ld8, s8, self.out8_scales.plane, self.out8_scales.R, int(self.out8_from)
                g.c_bscale_k0 = self.out8_scales.k0
        elif self.a_scale is not None or self.w_scale is not None or self.a_bscale is not None or self.out8 is not None:
            raise TypeError("a_scale / w_scale / block scales belong to fp8 problems")
        g.out_f32 = _is_f32(self.out, "out")
        g.C = _dev(self.out, "out")
        g.lda, g.ldw, g.ldc = lda, ldw, ldc
        g.strideA, g.strideC = sA, sC
        g.M, g.N, g.K, g.batch = M, N, K, Bt
        g.bias = _opt(self.bias, "bias", BF16)
        if self.bias is not None and self.bias.numel() != N:
            raise ValueError("bias length != N")
        rpb = self.rows_per_batch
        rows = rpb if rpb > 0 else M
        if self.gate is not None:
            gr, gc, gld = _rowmajor2d(self.gate, "gate")
            if gc < N or gr < Bt * (M // rows):
                raise ValueError("gate too small for this problem")
            g.gate = _dev(self.gate, "gate", F32)
            g.gate_ld = gld
        if self.res is not None:
            Br, rr, rc, ldr, sR = _batched(self.res, "res")
            if (Br, rr, rc) != (Bt, M, N) or self.res.dtype != self.out.dtype:
                raise ValueError("res must match out in shape and dtype")
            g.res = _dev(self.res, "res")
            g.ldr, g.strideR = ldr, sR
        if self.add2 is not None:
            B2, ar, ac, ld2, s2 = _batched(self.add2, "add2")
            if (B2, ar, ac) != (Bt, M, N):
                raise ValueError("add2 must match out in shape")
            g.add2 = _dev(self.add2, "add2", BF16)
            g.ld2, g.stride2 = ld2, s2
        if self.rowscale is not None:
            rsc = self.rowscale
            if rsc.dim() == 2 and rsc.shape == (Bt, rows) and rsc.stride(1) == 1 and Bt > 1:
                g.stride_rowscale = rsc.stride(0)                     # one mask per batch entry
            elif rsc.numel() != rows or not rsc.is_contiguous():
                raise ValueError("rowscale must be contiguous with rows_per_batch (or M) elements, or [batch, rows]")
            g.rowscale = _dev(rsc, "rowscale", F32)
        if self.rope is not None:
            r = self.rope
            if self.is_fp8:
                raise TypeError("the fused q/k RMSNorm + RoPE belongs to bf16 problems")
            if r.cos.shape != r.sin.shape or r.cos.dim() != 2 or r.cos.shape[1] != 128 or not r.cos.is_contiguous() or not r.sin.is_contiguous() \
                    or r.cos.shape[0] < r.pos0 + (rpb if rpb > 0 else M):
                raise ValueError("rope: cos/sin must be contiguous [positions,128] covering pos0 + rows")
            if r.wq.numel() != 128 or r.wk.numel() != 128:
                raise ValueError("rope: norm weights must have 128 elements")
            g.rope_cos, g.rope_sin = _dev(r.cos, "cos", F32), _dev(r.sin, "sin", F32)
            g.rope_wq, g.rope_wk = _dev(r.wq, "wq", BF16), _dev(r.wk, "wk", BF16)
            g.rope_q0, g.rope_k0, g.rope_w, g.rope_pos0, g.rope_eps = int(r.q0), int(r.k0), int(r.width), int(r.pos0), float(r.eps)
        g.rows_per_batch = rpb
        g.gelu_from = N if self.gelu_from is None else int(self.gelu_from)
        if 0 < g.gelu_from < N and g.gelu_from % 4:
            raise ValueError(f"gelu_from = {g.gelu_from}: a first GELU column inside (0, N) must be a multiple of 4 (the epilogue decides per 4-column group)")
        g.alpha = float(self.alpha)
        return g


def linear_grouped(problems: Sequence[LinearProblem]) -> None:
    """Enqueue up to RT_GEMM_MAX_GROUPS independent linears as ONE launch (image + text stream of a block)."""
    n = len(problems)
    if not 1 <= n <= native.RT_GEMM_MAX_GROUPS:
        raise ValueError(f"1..{native.RT_GEMM_MAX_GROUPS} problems per launch")
    arr = (native.GemmGroup * n)(*[p.to_group() for p in problems])
    fp8 = problems[0].is_fp8
    if any(p.is_fp8 != fp8 for p in problems):
        raise TypeError("all problems of one launch must have the same operand dtype")
    native.call("rt_gemm_fp8" if fp8 else "rt_gemm_bf16", arr, n, _stream())


def linear(a, w, out, **kw) -> torch.Tensor:
    linear_grouped([LinearProblem(a, w, out, **kw)])
    return out


def linear_skinny(hi: torch.Tensor, lo: torch.Tensor, problems: Sequence[tuple]) -> None:
    """out = lo @ w.T + (hi @ w.T + bias) for up to two (w, bias, out) problems that share hi / lo [M,K] bf16 (M <= 32), out f32
    [M,N]: ONE launch that streams every weight once; bit-identical to linear(hi, w, out, bias=bias); linear(lo, w, out, res=out)."""
    M, K, lda = _rowmajor2d(hi, "hi")
    if lo.shape != hi.shape or lo.stride() != hi.stride():
        raise ValueError("hi / lo must have the same shape and strides")
    n = len(problems)
    if not 1 <= n <= 2:
        raise ValueError("1..2 problems per launch")
    arr = (native.SkinnyGroup * n)()
    for g, (w, bias, out) in zip(arr, problems):
        N, Kw, ldw = _rowmajor2d(w, "w")
        Mo, No, ldc = _rowmajor2d(out, "out")
        if Kw != K or Mo != M or No != N or (bias is not None and bias.numel() != N):
            raise ValueError(f"linear_skinny shapes mismatch: hi{tuple(hi.shape)} w{tuple(w.shape)} out{tuple(out.shape)}")
        g.W, g.bias, g.C = _dev(w, "w", BF16), _opt(bias, "bias", BF16), _dev(out, "out", F32)
        g.ldw, g.ldc, g.N = ldw, ldc, N
    native.call("rt_gemm_skinny_bf16", _dev(hi, "hi", BF16), _dev(lo, "lo", BF16), lda, M, K, arr, n, _stream())


def add_rows_(y: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[r] = (y[r] + a[r % B]) + b[r % B] in place; y f32 [rows,D], a / b f32 [B,D], all contiguous."""
    rows, D = y.shape
    B = a.shape[0]
    if not y.is_contiguous() or not a.is_contiguous() or a.shape[1] != D or (b is not None and (b.shape != a.shape or not b.is_contiguous())):
        raise ValueError("add_rows_: y [rows,D], a / b [B,D], contiguous")
    native.call("rt_add_rows_f32", _dev(y, "y", F32), _dev(a, "a", F32), _opt(b, "b", F32), rows, B, D, _stream())
    return y


def gemv(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, silu_in=False,
         silu_out=False, accumulate=False) -> torch.Tensor:
    """out[b,n] (+)= post(sum_k pre(x[b,k]) w[n,k] + bias[n]); x,out f32, w,bias bf16."""
    B, K, ldx = _rowmajor2d(x, "x")
    N, Kw, ldw = _rowmajor2d(w, "w")
    Bo, No, ldy = _rowmajor2d(out, "out")
    if Kw != K or Bo != B or No != N:
        raise ValueError("gemv shapes mismatch")
    step = max(1, min(8, 16384 // K))      # rt_gemv_bf16w: at most 8 rows and 64 KiB of staged fp32 activations per launch; rows are independent
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        native.call("rt_gemv_bf16w", _dev(x, "x", F32) + b0 * ldx * 4, ldx, _dev(w, "w", BF16), ldw, _opt(bias, "bias", BF16),
                    _dev(out, "out", F32) + b0 * ldy * 4, ldy, nb, N, K, int(silu_in), int(silu_out), int(accumulate), _stream())
    return out


def timestep_embedding(t: torch.Tensor, dim: int = 256) -> torch.Tensor:
    t = t.contiguous()
    out = torch.empty(t.numel(), dim, device=t.device, dtype=F32)
    native.call("rt_timestep_embedding", _dev(t, "t", F32), out.data_ptr(), t.numel(), dim, _stream())
    return out


def rope_table(ids: torch.Tensor, axes_dim=(16, 56, 56), theta: float = 10000.0):
    ids = ids.to(F32).contiguous()
    S = ids.shape[0]
    D = int(sum(axes_dim))
    cos = torch.empty(S, D, device=ids.device, dtype=F32)
    sin = torch.empty(S, D, device=ids.device, dtype=F32)
    ax = (C.c_int32 * 3)(*[int(a) for a in axes_dim])
    native.call("rt_rope_table", _dev(ids, "ids", F32), cos.data_ptr(), sin.data_ptr(), S, ax, float(theta), _stream())
    return cos, sin


def layernorm_modulate(x: torch.Tensor, out: torch.Tensor, shift: Optional[torch.Tensor], scale: Optional[torch.Tensor],
                       eps: float = 1e-6) -> torch.Tensor:
    """x [B,R,D] (bf16|f32, unit inner stride) -> out [B,R,D] bf16 = LN(x)*(1+scale[b])+shift[b]; shift/scale f32 [B,D] views."""
    B, R, D, ldx, sxb = _rows3(x, "x")
    _, _, _, ldo, sob = _rows3(out, "out", shape=x.shape)
    mod_ld, x_f32 = _modulation(shift, scale, B, D), _is_f32(x)
    native.call("rt_layernorm_modulate", _dev(x, "x"), ldx, sxb, x_f32, _dev(out, "out", BF16), ldo, sob,
                _opt(shift, "shift", F32), _opt(scale, "scale", F32), mod_ld, B, R, D, float(eps), _stream())
    return out


def layernorm_modulate_pair(x0, out0, shift0, scale0, x1, out1, shift1, scale1, eps: float = 1e-6) -> None:
    """layernorm_modulate(x0, out0, shift0, scale0) and layernorm_modulate(x1, out1, shift1, scale1) as ONE launch (the image rows and
    the text rows of a double block): same dtype of x and same D, everything else per segment. Bit-identical to the two calls."""
    segs = (native.LnSegment * 2)()
    D, x_f32 = x0.shape[2], _is_f32(x0)
    for g, (x, out, shift, scale) in zip(segs, ((x0, out0, shift0, scale0), (x1, out1, shift1, scale1))):
        g.batch, g.rows_per_batch, _, g.ldx, g.stride_xb = _rows3(x, "x", width=D)
        _, _, _, g.ldo, g.stride_ob = _rows3(out, "out", shape=x.shape)
        if x.dtype != x0.dtype:
            raise ValueError("layernorm_modulate_pair: the two segments must have one dtype of x")
        g.mod_ld = _modulation(shift, scale, g.batch, D)
        g.x, g.out, g.shift, g.scale = _dev(x, "x"), _dev(out, "out", BF16), _opt(shift, "shift", F32), _opt(scale, "scale", F32)
    native.call("rt_layernorm_modulate_pair", segs, x_f32, D, float(eps), _stream())


def layernorm_modulate_fp8(x: torch.Tensor, out: torch.Tensor, row_scale: torch.Tensor, shift: Optional[torch.Tensor],
                           scale: Optional[torch.Tensor], eps: float = 1e-6) -> torch.Tensor:
    """As layernorm_modulate, quantising each modulated row to e4m3: out [B,R,D] float8_e4m3fn, row_scale f32 [B*R] contiguous
    (row b*R + r) — the A operand and a_scale of an fp8 LinearProblem."""
    B, R, D, ldx, sxb = _rows3(x, "x")
    _, _, _, ldo, sob = _rows3(out, "out", shape=x.shape)
    if row_scale.numel() != B * R or not row_scale.is_contiguous():
        raise ValueError("row_scale must be contiguous with B*R elements")
    mod_ld, x_f32 = _modulation(shift, scale, B, D), _is_f32(x)
    native.call("rt_layernorm_modulate_fp8", _dev(x, "x"), ldx, sxb, x_f32, _dev(out, "out", FP8), ldo, sob,
                _dev(row_scale, "row_scale", F32), _opt(shift, "shift", F32), _opt(scale, "scale", F32), mod_ld, B, R, D, float(eps), _stream())
    return out


def quantize_rows_fp8(x: torch.Tensor):
    """x [rows, D] bf16|f32 (unit inner stride) -> (e4m3 [rows, D], scale f32 [rows]) with x ≈ q * scale[:, None]."""
    rows, D, ldx = _rowmajor2d(x, "x")
    x_f32 = _is_f32(x)
    q = torch.empty(rows, D, device=x.device, dtype=FP8)
    sc = torch.empty(rows, device=x.device, dtype=F32)
    native.call("rt_quantize_rows_fp8", _dev(x, "x"), ldx, x_f32, q.data_ptr(), D, sc.data_ptr(), rows, D, _stream())
    return q, sc


def quantize_rows_fp8_into(x: torch.Tensor, out: torch.Tensor, scale: torch.Tensor) -> None:
    """x [B,R,D] bf16|f32 view (unit inner stride, any row / batch stride) -> out [B,R,D] e4m3 view, scale f32 [B*R] contiguous
    (row b*R + r): the A operand and a_scale of an fp8 LinearProblem for activations that do not come out of a LayerNorm."""
    B, R, D, ldx, sxb = _rows3(x, "x")
    _, _, _, ldo, sob = _rows3(out, "out", shape=x.shape)
    if scale.numel() != B * R or not scale.is_contiguous():
        raise ValueError("scale must be contiguous with B*R elements")
    x_f32, esz, st = _is_f32(x), x.element_size(), _stream()
    po, ps, px = _dev(out, "out", FP8), _dev(scale, "scale", F32), _dev(x, "x")
    for b in range(B):
        native.call("rt_quantize_rows_fp8", px + b * sxb * esz, ldx, x_f32, po + b * sob, ldo, ps + b * R * 4, R, D, st)


def quantize_mx_fp8_into(x: torch.Tensor, out: torch.Tensor, scales: BlockScales) -> None:
    """x [B,R,D] bf16|f32 view -> out [B,R,D] e4m3 view + E8M0 block scales (one per 32 elements, rt_quantize_mx_fp8): the A operand
    and a_bscale of an fp8 LinearProblem for tensors no fused producer writes."""
    B, R, D, ldx, sxb = _rows3(x, "x")
    _, _, _, ldo, sob = _rows3(out, "out", shape=x.shape)
    x_f32, esz, st = _is_f32(x), x.element_size(), _stream()
    if D % 256 or scales.k0 != 0 or scales.columns_left() < D:
        raise ValueError("D % 256 == 0, written from column 0 of a scale tensor that covers D")
    po, px = _dev(out, "out", FP8), _dev(x, "x")
    for b in range(B):
        native.call("rt_quantize_mx_fp8", px + b * sxb * esz, ldx, x_f32, po + b * sob, ldo,
                    scales.ptr() + b * (scales.R // 64) * 2048, scales.plane, R, D, st)


def dequantize_mx(q: torch.Tensor, scales: BlockScales) -> torch.Tensor:
    """fp32 [B,R,D] value of an e4m3 tensor with block scales (host-side helper for tests and tools; torch ops)."""
    B, R, D = q.shape
    e = scales.rowmajor(B, R, D).to(torch.float32) - 127.0
    return (q.to(torch.float32).view(B, R, D // 32, 32) * torch.exp2(e).unsqueeze(-1)).view(B, R, D)


def lora_merge_(w: torch.Tensor, w0: torch.Tensor, terms: Sequence[tuple]) -> torch.Tensor:
    """w = bf16(w0 + Σ c·B·A) (rt_lora_merge_bf16): ``terms`` = (B [N, r_pad] bf16, At [K, r_pad] bf16, c) with the r columns
    zero-padded to a multiple of 32 and A stored transposed. w / w0 [N, K] bf16 views with unit inner stride (rows of a fused
    weight are fine); w may be w0. No terms: w0 is copied bit for bit. One launch on the current stream."""
    N, K, ldw = _rowmajor2d(w, "w")
    N0, K0, ld0 = _rowmajor2d(w0, "w0")
    if (N0, K0) != (N, K):
        raise ValueError(f"lora_merge_: w {tuple(w.shape)} and w0 {tuple(w0.shape)} differ")
    if len(terms) > native.RT_LORA_MAX_TERMS:
        raise ValueError(f"lora_merge_: at most {native.RT_LORA_MAX_TERMS} terms per weight, got {len(terms)}")
    if K % 8 or ldw % 8 or ld0 % 8:
        raise ValueError("lora_merge_: K and the row strides must be multiples of 8")
    pw, p0 = _dev(w, "w", BF16), _dev(w0, "w0", BF16)
    arr = (native.LoraTerm * max(1, len(terms)))()
    for t, (b, at, c) in enumerate(terms):
        rb, r_pad, ldb = _rowmajor2d(b, "B")
        ka, ra, lda = _rowmajor2d(at, "At")
        if rb != N or ka != K or ra != r_pad or r_pad % 32:
            raise ValueError(f"lora_merge_: term {t}: B {tuple(b.shape)} / At {tuple(at.shape)} do not fit w [{N}, {K}] with r_pad % 32 == 0")
        if b.device != w.device or at.device != w.device:
            raise RuntimeError("lora_merge_: factors and weight must be on the same device")
        arr[t] = native.LoraTerm(_dev(b, "B", BF16), _dev(at, "At", BF16), ldb, lda, r_pad, float(c))
    native.call("rt_lora_merge_bf16", arr, len(terms), p0, ld0, pw, ldw, N, K, _stream())
    return w


def qk_rmsnorm_rope(buf: torch.Tensor, q_off: int, k_off: int, H: int, T: int, wq_txt, wk_txt, wq_img, wk_img,
                    cos: torch.Tensor, sin: torch.Tensor, eps: float = 1e-6) -> None:
    """In place on buf [B,S,ld] bf16: heads at columns q_off + h*128 / k_off + h*128."""
    B, S, _, ld, sb = _rows3(buf, "buf")
    if cos.shape != (S, 128) or sin.shape != (S, 128) or not cos.is_contiguous() or not sin.is_contiguous():
        raise ValueError("cos/sin must be contiguous [S,128]")
    native.call("rt_qk_rmsnorm_rope", _dev(buf, "buf", BF16), ld, sb, q_off, k_off, _opt(wq_txt, "wq_txt", BF16), _opt(wk_txt, "wk_txt", BF16),
                _dev(wq_img, "wq_img", BF16), _dev(wk_img, "wk_img", BF16), _dev(cos, "cos", F32), _dev(sin, "sin", F32), B, S, T, H, float(eps), _stream())


_ATTN_WS = {}
CAPTURE_KEEP: Optional[list] = None      # see mmdit.CAPTURE_KEEP: workspaces a graph under capture refers to


def _attention_workspace(B: int, S: int, H: int, device) -> Optional[torch.Tensor]:
    """Workspace of rt_attention_fwd's key-split tail (ticket counters + partial records), one per (shape, device, stream):
    two streams may run attention of the same shape at once (tower beside transformer). Zeroed once — the kernel leaves the
    counters zero. None when this shape splits nothing. A workspace first requested while a stream capture is running is
    zeroed by a memset NODE of that graph (replayed with it); should the capture be abandoned, pipeline._denoise drops the
    entries it created (drop_attention_workspaces), so a never-executed zero fill cannot be picked up later."""
    key = (B, S, H, str(device), _stream())
    ws = _ATTN_WS.get(key, False)
    if ws is False:
        n = int(native.load().rt_attention_ws_bytes(B, S, H))
        ws = torch.zeros(n, device=device, dtype=torch.uint8) if n > 0 else None
        if len(_ATTN_WS) > 16:
            _ATTN_WS.clear()
        _ATTN_WS[key] = ws
    if CAPTURE_KEEP is not None and ws is not None:
        CAPTURE_KEEP.append(ws)
    return ws


def drop_attention_workspaces(keys) -> None:
    for k in list(keys):
        _ATTN_WS.pop(k, None)


@dataclass(frozen=True)
class KeyGroups:
    """Key groups of a region-masked attention call (rt_attention_fwd_grouped). ``ends``: ascending key indices, group g = keys
    [ends[g-1], ends[g]); at most 32, the last equals S, all others are multiples of 64. ``row_vis``: int32 or uint32 [B or 1, S] on the
    device; query row i of entry b attends the keys of group g iff bit g of row_vis[b, i] is set ([1, S]: one table for the batch)."""
    ends: tuple
    row_vis: torch.Tensor

    def check(self, B: int, S: int) -> Tuple[int, int]:
        """Validate against a [B, S, .] call; returns (row_vis pointer, its batch stride in words)."""
        ends = tuple(int(e) for e in self.ends)
        if not 1 <= len(ends) <= 32:
            raise ValueError(f"groups: need 1..32 key groups, got {len(ends)}")
        if any(b <= a for a, b in zip((0,) + ends, ends)):
            raise ValueError(f"groups: ends must be positive and ascending, got {ends}")
        if any(e % 64 for e in ends[:-1]):
            raise ValueError(f"groups: every end but the last must be a multiple of 64, got {ends}")
        if ends[-1] != S:
            raise ValueError(f"groups: the last end must be S = {S}, got {ends[-1]}")
        rv = self.row_vis
        if not isinstance(rv, torch.Tensor) or rv.dtype not in (torch.int32, torch.uint32):
            raise TypeError("groups.row_vis must be an int32 or uint32 tensor")
        if rv.dim() != 2 or rv.shape[1] != S or rv.shape[0] not in (1, B) or rv.stride(1) != 1:
            raise ValueError(f"groups.row_vis: need [{B} or 1, {S}] with unit inner stride, got {tuple(rv.shape)} / {rv.stride()}")
        return _dev(rv, "groups.row_vis"), (0 if rv.shape[0] == 1 else rv.stride(0))


@dataclass(frozen=True)
class KeyClasses:
    """Key classes of a per-key masked attention call (rt_attention_fwd_keyed). ``key_class``: uint8 [B or 1, S], the class id 0..31 of
    every key; ``row_vis``: int32 or uint32 [B or 1, S]; query row i of entry b attends key j iff bit key_class[b, j] of row_vis[b, i] is
    set. Dtypes, ranks and unit inner strides are checked here, once; so are the class ids (< 32) when the record is built from host
    tensors — ``to(device)`` then gives the record the launch takes. A record built from device tensors (a captured loop's own
    clones) is not read back. The entry reads the byte table a byte at a time: nothing is padded or re-laid."""
    row_vis: torch.Tensor
    key_class: torch.Tensor

    def __post_init__(self):
        rv, kc = self.row_vis, self.key_class
        if not isinstance(rv, torch.Tensor) or rv.dtype not in (torch.int32, torch.uint32):
            raise TypeError("groups.row_vis must be an int32 or uint32 tensor")
        if not isinstance(kc, torch.Tensor) or kc.dtype != torch.uint8:
            raise TypeError("groups.key_class must be a uint8 tensor")
        if rv.dim() != 2 or kc.dim() != 2 or rv.shape[1] != kc.shape[1] or rv.stride(1) != 1 or kc.stride(1) != 1:
            raise ValueError(f"groups: row_vis and key_class must be [B or 1, S] with unit inner stride, got {tuple(rv.shape)} / {rv.stride()} "
                             f"and {tuple(kc.shape)} / {kc.stride()}")
        if kc.device.type == "cpu" and kc.numel() and int(kc.max()) > 31:
            raise ValueError(f"groups.key_class: class ids must be below 32, got {int(kc.max())}")

    def to(self, device) -> "KeyClasses":
        return KeyClasses(self.row_vis.to(device), self.key_class.to(device))

    def check(self, B: int, S: int) -> Tuple[int, int, int, int]:
        """Validate against a [B, S, .] call; returns (row_vis pointer, its batch stride in words, key_class pointer, its batch stride
        in bytes)."""
        rv, kc = self.row_vis, self.key_class
        for name, t in (("row_vis", rv), ("key_class", kc)):
            if t.shape[1] != S or t.shape[0] not in (1, B):
                raise ValueError(f"groups.{name}: need [{B} or 1, {S}], got {tuple(t.shape)}")
        return (_dev(rv, "groups.row_vis"), (0 if rv.shape[0] == 1 else rv.stride(0)),
                _dev(kc, "groups.key_class"), (0 if kc.shape[0] == 1 else kc.stride(0)))


def _key_bias(kb, B: int, device) -> Tuple[int, int]:
    """Validate ``attention``'s ``key_bias`` against a batch of B -> (pointer, batch stride in elements; 0: one table)."""
    if not isinstance(kb, torch.Tensor) or kb.dtype != F32:
        raise TypeError("attention: key_bias must be a float32 tensor")
    if kb.dim() != 2 or kb.shape[1] != 32 or kb.shape[0] not in (1, B) or kb.stride(1) != 1:
        raise ValueError(f"attention: key_bias: need [{B} or 1, 32] with unit inner stride, got {tuple(kb.shape)} / {kb.stride()}")
    if kb.device != device:
        raise RuntimeError(f"attention: key_bias is on {kb.device}, q on {device}")
    return _dev(kb, "key_bias", F32), (0 if kb.shape[0] == 1 else kb.stride(0))


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int, scale: Optional[float] = None,
              split: bool = True, rows: Optional[tuple] = None, groups: Optional[Union[KeyGroups, KeyClasses]] = None,
              key_bias: Optional[torch.Tensor] = None, self_key: bool = False) -> torch.Tensor:
    """q,k,v [B,S,H*128] views (common strides) of one buffer; out [B,S,H*128] view (may alias q). ``split=False`` runs every
    128-row block as one full-length workgroup (no key-split tail; A/B and tests). ``rows`` = (r0, r1): only the items of the launch that
    hold a query row of [r0, r1) do any work (rt_attention_fwd_rows): those rows of out get the bits the whole launch gives them, the
    other rows of the touched items are written too, the rest of out is left as it is. ``groups`` (a KeyGroups; not together with
    ``rows``): region-masked attention, rt_attention_fwd_grouped — hidden keys must still hold finite values; a KeyClasses in its
    place: visibility per key, rt_attention_fwd_keyed. ``key_bias`` (only with ``groups``): float32 [B or 1, 32] on q's device, added
    to the logits (natural-log units) of the keys of group / class c — the softmax weight of those keys times exp(key_bias[b, c]); finite
    values; visibility is unchanged (rt_attention_fwd_grouped_biased / rt_attention_fwd_keyed_biased). None: the unbiased entries.
    ``self_key=True`` (only with a KeyClasses, without ``rows`` and ``key_bias``): row i also sees key i whatever its word says,
    rt_attention_fwd_keyed_self (perturbed-attention guidance)."""
    (B, S, _, ld, sb), _, _, (_, _, _, ldo, sob) = [_rows3(t, name, width=H * 128) for name, t in (("q", q), ("k", k), ("v", v), ("out", out))]
    if not (q.stride() == k.stride() == v.stride()) or k.shape != q.shape or v.shape != q.shape or out.shape != q.shape:
        raise ValueError("q,k,v must share shape and strides")
    sc = (128 ** -0.5) if scale is None else float(scale)
    if key_bias is not None and groups is None:
        raise ValueError("attention: key_bias= needs groups= (a bias per key group or class)")
    if self_key and (not isinstance(groups, KeyClasses) or rows is not None or key_bias is not None):
        raise ValueError("attention: self_key=True needs groups= as a KeyClasses (the self rule belongs to the per-key launch), "
                         "without rows= and key_bias=")
    if groups is not None:
        if rows is not None:
            raise ValueError("attention: rows= and groups= cannot be combined")
        if not sc > 0:
            raise ValueError("attention: groups= needs scale > 0")
        if isinstance(groups, KeyClasses):
            vis, svb, cls, scb = groups.check(B, S)
            bias = None if key_bias is None else _key_bias(key_bias, B, q.device)
            ws = _attention_workspace(B, S, H, q.device) if split else None
            if bias is not None:
                native.call("rt_attention_fwd_keyed_biased", _dev(q, "q", BF16), _dev(k, "k", BF16), _dev(v, "v", BF16), _dev(out, "out", BF16),
                            ld, sb, ldo, sob, B, S, H, sc, vis, svb, cls, scb, None if ws is None else ws.data_ptr(),
                            0 if ws is None else ws.numel(), _stream(), *bias)
                return out
            native.call("rt_attention_fwd_keyed_self" if self_key else "rt_attention_fwd_keyed", _dev(q, "q", BF16), _dev(k, "k", BF16), _dev(v, "v", BF16), _dev(out, "out", BF16), ld,
                        sb, ldo, sob, B, S, H, sc, vis, svb, cls, scb, None if ws is None else ws.data_ptr(),
                        0 if ws is None else ws.numel(), _stream())
            return out
        vis, svb = groups.check(B, S)
        ends = (C.c_int32 * len(groups.ends))(*[int(e) for e in groups.ends])
        bias = None if key_bias is None else _key_bias(key_bias, B, q.device)
        ws = _attention_workspace(B, S, H, q.device) if split else None
        if bias is not None:
            native.call("rt_attention_fwd_grouped_biased", _dev(q, "q", BF16), _dev(k, "k", BF16), _dev(v, "v", BF16), _dev(out, "out", BF16),
                        ld, sb, ldo, sob, B, S, H, sc, C.cast(ends, C.c_void_p), len(groups.ends), vis, svb,
                        None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), _stream(), *bias)
            return out
        native.call("rt_attention_fwd_grouped", _dev(q, "q", BF16), _dev(k, "k", BF16), _dev(v, "v", BF16), _dev(out, "out", BF16), ld, sb,
                    ldo, sob, B, S, H, sc, C.cast(ends, C.c_void_p), len(groups.ends), vis, svb,
                    None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), _stream())
        return out
    ws = _attention_workspace(B, S, H, q.device) if split else None
    r0, r1 = (0, S) if rows is None else (int(rows[0]), int(rows[1]))
    native.call("rt_attention_fwd_rows", _dev(q, "q", BF16), _dev(k, "k", BF16), _dev(v, "v", BF16), _dev(out, "out", BF16), ld, sb,
                ldo, sob, B, S, H, sc, r0, r1, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), _stream())
    return out


def ip_attention(q: torch.Tensor, wq: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int, ip_scale: float = 1.0,
                 accumulate: bool = False, scale: Optional[float] = None, eps: float = 1e-6,
                 row_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (+)= ip_scale · softmax(bf16(rmsnorm(q)·wq) Kᵀ · scale) V (rt_ip_attention): the IP-Adapter term of a double block.
    q [B,N,H·128] bf16 view of the RAW query projection (unit inner stride, e.g. columns :d of the fused q|k|v buffer; not modified);
    wq bf16 [128] (norm_q.weight); k, v [B or 1, n, H·128] bf16 views sharing strides, 1 <= n <= 128 (batch 1: one image prompt for
    every batch entry); out [B,N,H·128] bf16 or f32 view. The launch is ip_attention_gated's without a gate, to which the C entry
    rt_ip_attention itself forwards."""
    return ip_attention_gated(q, wq, k, v, out, H, ip_scale, None, accumulate, scale, eps, row_weights)


def ip_attention_gated(q: torch.Tensor, wq: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int, ip_scale: float = 1.0,
                       gate: Optional[torch.Tensor] = None, accumulate: bool = False, scale: Optional[float] = None, eps: float = 1e-6,
                       row_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (+)= gate[b] · ip_scale · softmax(bf16(rmsnorm(q)·wq) Kᵀ · scale) V (rt_ip_attention_gated): ip_attention with an optional
    fp32 column gate [B, H·128] (a view with unit inner stride and any batch stride, e.g. the gate_msa chunk of the modulation table).
    q may be any [B,rows,H·128] view (a single block: columns 2d:3d of the fused [k|v|q|mlp] buffer, all S rows); k as given.
    row_weights: fp32 [B or 1, rows] with unit inner stride, a weight per query row multiplied into ip_scale (rt_ip_attention_rows: a
    row of weight 0 is left alone when accumulating and written as +0 otherwise, and tiles of such rows cost nothing); None is the
    launch without weights."""
    d = H * 128
    (B, N, _, ldq, sqb), (Bk, n, _, ldkv, skvb), _, (_, _, _, ldo, sob) = [_rows3(t, name, width=d) for name, t in (("q", q), ("k", k), ("v", v), ("out", out))]
    if out.shape != q.shape or out.dtype not in (BF16, F32):
        raise ValueError("out must match q in shape and be bf16 or f32")
    if k.shape != v.shape or k.stride() != v.stride() or Bk not in (1, B):
        raise ValueError("k and v must share shape and strides, with batch 1 or B")
    if not 1 <= n <= 128:
        raise ValueError(f"ip_attention_gated: 1..128 image-prompt tokens, got {n}")
    if wq.numel() != 128 or not wq.is_contiguous():
        raise ValueError("wq must be contiguous with 128 elements")
    if gate is not None and (gate.dim() != 2 or gate.shape != (B, d) or gate.stride(1) != 1):
        raise ValueError(f"gate must be a [B,{d}] view with unit inner stride")
    sc = (128 ** -0.5) if scale is None else float(scale)
    if row_weights is not None:
        if row_weights.dim() != 2 or row_weights.shape[0] not in (1, B) or row_weights.shape[1] != N or row_weights.stride(1) != 1:
            raise ValueError(f"row_weights must be a [B or 1,{N}] view with unit inner stride")
        swb = row_weights.stride(0) if row_weights.shape[0] == B and B > 1 else 0
        native.call("rt_ip_attention_rows", _dev(q, "q", BF16), ldq, sqb, _dev(wq, "wq", BF16), _dev(k, "k", BF16), _dev(v, "v", BF16), ldkv,
                    skvb if Bk == B and B > 1 else 0, _opt(gate, "gate", F32), 0 if gate is None else gate.stride(0),
                    _dev(row_weights, "row_weights", F32), swb, _dev(out, "out"), ldo, sob, int(out.dtype == F32), int(accumulate), B, N, H, n, sc,
                    float(ip_scale), float(eps), _stream())
        return out
    native.call("rt_ip_attention_gated", _dev(q, "q", BF16), ldq, sqb, _dev(wq, "wq", BF16), _dev(k, "k", BF16), _dev(v, "v", BF16), ldkv,
                skvb if Bk == B and B > 1 else 0, _opt(gate, "gate", F32), 0 if gate is None else gate.stride(0),
                _dev(out, "out"), ldo, sob, int(out.dtype == F32), int(accumulate), B, N, H, n, sc, float(ip_scale), float(eps), _stream())
    return out


def gelu_erf(x: torch.Tensor) -> torch.Tensor:
    """bf16(exact GELU(x)) of a contiguous f32 tensor (rt_gelu_erf_bf16)."""
    if not x.is_contiguous():
        raise ValueError("gelu_erf: contiguous input")
    out = torch.empty(x.shape, device=x.device, dtype=BF16)
    native.call("rt_gelu_erf_bf16", _dev(x, "x", F32), out.data_ptr(), x.numel(), _stream())
    return out


def add_bf16_(y: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """y = bf16(y + x) in place on [B,R,D] bf16 views with unit inner stride and any row / batch strides (rt_add_bf16_2d)."""
    B, R, D, ldx, sxb = _rows3(x, "x")
    _, _, _, ldy, syb = _rows3(y, "y", shape=x.shape)
    native.call("rt_add_bf16_2d", _dev(x, "x", BF16), ldx, sxb, _dev(y, "y", BF16), ldy, syb, B, R, D, _stream())
    return y


def rmsnorm_heads_(x: torch.Tensor, out: torch.Tensor, ones: torch.Tensor, eps: float) -> torch.Tensor:
    """out = bf16(x · rsqrt(mean_128(x²) + eps)) per group of 128 consecutive elements (rt_rmsnorm_rows with a weight of ones, which
    multiplies exactly): x contiguous f32, out contiguous bf16 of the same shape, numel % 128 == 0."""
    if x.shape != out.shape or not x.is_contiguous() or not out.is_contiguous() or x.numel() % 128 or ones.numel() != 128:
        raise ValueError("rmsnorm_heads_: contiguous tensors of equal shape, a multiple of 128 elements")
    native.call("rt_rmsnorm_rows", _dev(x, "x", F32), 128, 1, _dev(ones, "ones", BF16), _dev(out, "out", BF16), 128,
                x.numel() // 128, 128, float(eps), _stream())
    return out


def _attention_small_head(hd: int, entry: str, max_s: int, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int,
                          scale: Optional[float]) -> torch.Tensor:
    """The body of attention_hd64 / attention_hd72 (csrc/attention_small_head.hip): head dim, entry point and row bound. 64 keeps its
    stricter rule — q, k and v are views of one buffer sharing shape and strides — which its entry point's shorter argument list assumes."""
    d = H * hd
    (Bq, Sq, _, ldq, sqb), (B, Sk, _, ldkv, skvb), _, (_, _, _, ldo, sob) = [_rows3(t, name, width=d) for name, t in (("q", q), ("k", k), ("v", v), ("out", out))]
    sc = float(scale if scale is not None else (64 ** -0.5 if hd == 64 else 72 ** -0.5))      # literals: folded when compiled
    if hd == 64:
        if not (q.stride() == k.stride() == v.stride()) or k.shape != q.shape or v.shape != q.shape or out.shape != q.shape:
            raise ValueError("q,k,v must share shape and strides; out must have their shape")
        if not 1 <= Sq <= max_s:
            raise ValueError(f"{entry[3:]}: 1..{max_s} rows, got {Sq}")
        native.call(entry, _dev(q, "q", BF16), _dev(k, "k", BF16), _dev(v, "v", BF16), ldq, sqb, _dev(out, "out", BF16), ldo, sob, B, Sq, H, sc, _stream())
    else:
        if k.stride() != v.stride() or v.shape != k.shape:
            raise ValueError("k,v must share shape and strides")
        if Bq not in (1, B) or out.shape != (B, Sq, d):
            raise ValueError(f"q must be [{B} or 1, Sq, {d}] and out [{B}, Sq, {d}], got {tuple(q.shape)} and {tuple(out.shape)}")
        if not (1 <= Sq <= max_s and 1 <= Sk <= max_s):
            raise ValueError(f"{entry[3:]}: 1..{max_s} rows, got {Sq} queries and {Sk} keys")
        native.call(entry, _dev(q, "q", BF16), ldq, sqb if Bq == B and B > 1 else 0, _dev(k, "k", BF16), _dev(v, "v", BF16), ldkv, skvb,
                    _dev(out, "out", BF16), ldo, sob, B, Sq, Sk, H, sc, _stream())
    return out


def attention_hd64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int, scale: Optional[float] = None) -> torch.Tensor:
    """out[b, s, h·64:(h+1)·64] = softmax(scale · q_h k_hᵀ) v_h (rt_attention_hd64): non-causal self-attention with heads of 64, one
    launch. q, k, v [B,S,H·64] bf16 views of one buffer sharing strides (the fused q|k|v projection); out [B,S,H·64] bf16 view with its
    own strides; 1 <= S <= native.RT_ATTENTION_HD64_MAX_S."""
    return _attention_small_head(64, "rt_attention_hd64", native.RT_ATTENTION_HD64_MAX_S, q, k, v, out, H, scale)


def attention_hd72(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int, scale: Optional[float] = None) -> torch.Tensor:
    """out[b, s, h·72:(h+1)·72] = softmax(scale · q_h k_hᵀ) v_h (rt_attention_hd72): non-causal attention with heads of 72, one launch.
    q [B or 1, Sq, H·72] bf16 (a leading 1 is shared by the batch: the pooling head's probe); k, v [B, Sk, H·72] bf16 views sharing
    shape and strides (the fused projection); out [B, Sq, H·72] bf16 view with its own strides; 1 <= Sq, Sk <= native.RT_ATTENTION_HD72_MAX_S."""
    return _attention_small_head(72, "rt_attention_hd72", native.RT_ATTENTION_HD72_MAX_S, q, k, v, out, H, scale)


def patchify_nchw(x: torch.Tensor, patch: int, Kp: Optional[int] = None) -> torch.Tensor:
    """im2col of a stride-p, kernel-p convolution (rt_patchify_nchw): x [B,3,G·p,G·p] f32 or bf16 -> bf16 [B, G², Kp] with
    row[gy·G + gx][c·p² + dy·p + dx] = x[b, c, gy·p + dy, gx·p + dx] and zero columns from 3p² up to Kp (default: 3p² rounded up to 64)."""
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[2] % patch or x.dtype not in (BF16, F32):
        raise ValueError(f"patchify_nchw: need a square f32 or bf16 [B,3,G*{patch},G*{patch}] image, got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    B, G = x.shape[0], x.shape[2] // patch
    Kp = (3 * patch * patch + 63) // 64 * 64 if Kp is None else int(Kp)
    out = torch.empty(B, G * G, Kp, device=x.device, dtype=BF16)
    native.call("rt_patchify_nchw", _dev(x, "x"), int(x.dtype == F32), out.data_ptr(), B, G, patch, Kp, _stream())
    return out


def attention_fp8_prep(buf: torch.Tensor, q_off: int, k_off: int, v_off: int, H: int, T: int, wq_txt, wk_txt, wq_img, wk_img,
                       cos: torch.Tensor, sin: torch.Tensor, qk8: torch.Tensor, vt8: torch.Tensor, eps: float = 1e-6) -> None:
    """From the fused projection buffer buf [B,S,ld] bf16 (not modified): qk8 [B,S,2·H·128] e4m3 = 16 · RoPE(RMSNorm(q | k)),
    vt8 flat e4m3 of rt_attention_fp8_vt_bytes(B,S,H) bytes = Vᵀ per (batch, head), keys in MFMA operand order."""
    B, S, _, ld, sb = _rows3(buf, "buf")
    if cos.shape != (S, 128) or sin.shape != (S, 128) or not cos.is_contiguous() or not sin.is_contiguous():
        raise ValueError("cos/sin must be contiguous [S,128]")
    if qk8.shape != (B, S, 2 * H * 128) or not qk8.is_contiguous() or vt8.numel() < int(native.load().rt_attention_fp8_vt_bytes(B, S, H)):
        raise ValueError("qk8 must be contiguous [B,S,2*H*128]; vt8 must hold rt_attention_fp8_vt_bytes(B,S,H) bytes")
    native.call("rt_attention_fp8_prep", _dev(buf, "buf", BF16), ld, sb, q_off, k_off, v_off, _opt(wq_txt, "wq_txt", BF16), _opt(wk_txt, "wk_txt", BF16),
                _dev(wq_img, "wq_img", BF16), _dev(wk_img, "wk_img", BF16), _dev(cos, "cos", F32), _dev(sin, "sin", F32),
                _dev(qk8, "qk8", FP8), _dev(vt8, "vt8", FP8), B, S, T, H, float(eps), _stream())


def attention_fp8(qk8: torch.Tensor, vt8: torch.Tensor, out: torch.Tensor, H: int, scale: Optional[float] = None) -> torch.Tensor:
    """softmax(q kᵀ · scale) v from attention_fp8_prep's buffers -> out [B,S,>=H*128] bf16 view (unit inner stride)."""
    B, S, _ = qk8.shape
    Bo, So, _, ldo, sob = _rows3(out, "out")
    if (Bo, So) != (B, S):
        raise ValueError("out must be [B,S,*] with qk8's B and S")
    native.call("rt_attention_fp8_fwd", _dev(qk8, "qk8", FP8), _dev(vt8, "vt8", FP8), _dev(out, "out", BF16), ldo, sob, B, S, H,
                float(scale if scale is not None else 128 ** -0.5), _stream())
    return out


def attention_fp8_mx(qk8: torch.Tensor, vt8: torch.Tensor, out8: torch.Tensor, scales: BlockScales, H: int, scale: Optional[float] = None) -> torch.Tensor:
    """attention_fp8 with the output as e4m3 + E8M0 block scales (rt_attention_fp8_fwd_mx): out8 [B,S,>=H*128] e4m3 view, head h at
    columns h*128.. of the view; ``scales`` addresses the same view."""
    B, S, _ = qk8.shape
    Bo, So, _, ldo, sob = _rows3(out8, "out8")
    if (Bo, So) != (B, S):
        raise ValueError("out8 must be [B,S,*] with qk8's B and S")
    if scales.columns_left() < H * 128:
        raise ValueError("the scale tensor must cover the H*128 output columns")
    native.call("rt_attention_fp8_fwd_mx", _dev(qk8, "qk8", FP8), _dev(vt8, "vt8", FP8), _dev(out8, "out8", FP8), ldo, sob,
                scales.ptr(), scales.plane, scales.R, scales.k0, B, S, H, float(scale if scale is not None else 128 ** -0.5), _stream())
    return out8


def euler_step_(x: torch.Tensor, v: torch.Tensor, dsigma: float) -> torch.Tensor:
    if not (x.is_contiguous() and v.is_contiguous()) or x.shape != v.shape:
        raise ValueError("euler_step_: contiguous tensors of equal shape")
    native.call("rt_euler_step", _dev(x, "x", BF16), _dev(v, "v", BF16), float(dsigma), x.numel(), _stream())
    return x


def _check_master_step(name: str, x32: torch.Tensor, like, x_bf16: Optional[torch.Tensor], src32: Optional[torch.Tensor],
                       noise32: Optional[torch.Tensor], mask: Optional[torch.Tensor], contiguous=()) -> None:
    """The argument checks of every fp32 master step (``name``, for the messages): what is given of ``like``, src32 and noise32 has
    x32's shape and is contiguous, as are ``contiguous`` and the mask, which has x32's shape or that of one sample; x_bf16 matches x32."""
    if mask is not None and (src32 is None or noise32 is None):
        raise ValueError(f"{name}: a mask needs src32 and noise32")
    like = [t for t in (*like, src32, noise32) if t is not None]
    if not all(t.is_contiguous() for t in [x32, *contiguous, *like] + ([] if mask is None else [mask])) or not all(t.shape == x32.shape for t in like):
        raise ValueError(f"{name}: contiguous tensors of equal shape")
    if x_bf16 is not None and (x_bf16.shape != x32.shape or not x_bf16.is_contiguous()):
        raise ValueError("x_bf16 must match x32")
    if mask is not None and mask.shape != x32.shape and not (x32.dim() > 1 and tuple(mask.shape) == (1,) + tuple(x32.shape[1:])):
        raise ValueError(f"{name}: mask {tuple(mask.shape)} is neither x32's shape {tuple(x32.shape)} nor that of one sample")


def _master_step_f32(name: str, x32: torch.Tensor, v: torch.Tensor, v_text: Optional[torch.Tensor], s: float, dsigma: float,
                     x_bf16: Optional[torch.Tensor], sigma_next: float = 0.0, src32: Optional[torch.Tensor] = None,
                     noise32: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None,
                     w: float = 0.0, stochastic: Optional[StochasticArgs] = None) -> torch.Tensor:
    """The body of euler_step_f32_ / cfg_euler_step_f32_ / repaint_euler_step_f32_ / multistep_step_f32_ / stochastic_step_f32_
    (``name``, for the messages): the checks, and the entry that what is given selects. One fp32 master step x32 += dsigma·vel,
    vel = v or v + s·(v_text − v); with a mask, the blend; with ``hist`` (the fp32 velocity of the step before, replaced by this
    step's), vel + w·(vel − hist) in vel's place; with ``stochastic``, its rule in the Euler rule's place (``dsigma`` is then unused)."""
    _check_master_step(name, x32, (v, v_text, hist), x_bf16, src32, noise32, mask)
    if stochastic is not None:
        if hist is not None:
            raise ValueError(f"{name}: the stochastic step keeps no history (solver order 1 only)")
        B, n_s = _stochastic_batch(name, x32, stochastic, sigma_next)
    x, xb, n = _dev(x32, "x32", F32), _opt(x_bf16, "x_bf16", BF16), x32.numel()
    if stochastic is not None:
        native.call("rt_stochastic_step_f32", x, _dev(v, "v", BF16), _opt(v_text, "v_text", BF16), xb,
                    _opt(src32 if mask is not None else None, "src32", F32), _opt(noise32 if mask is not None else None, "noise32", F32),
                    _opt(mask, "mask", F32), _opt(stochastic.rng, "rng", torch.int64), float(s), *stochastic.scalars(sigma_next), B, n_s,
                    n if mask is None else mask.numel(), _stream())
    elif hist is not None:
        native.call("rt_multistep_step_f32", x, _dev(v, "v", BF16), _opt(v_text, "v_text", BF16), xb, _dev(hist, "hist", F32), float(w),
                    _opt(src32 if mask is not None else None, "src32", F32), _opt(noise32 if mask is not None else None, "noise32", F32),
                    _opt(mask, "mask", F32), float(s), float(dsigma), float(sigma_next), n, n if mask is None else mask.numel(), _stream())
    elif mask is not None:
        native.call("rt_repaint_euler_step_f32", x, _dev(v, "v", BF16), _opt(v_text, "v_text", BF16), xb, _dev(src32, "src32", F32),
                    _dev(noise32, "noise32", F32), _dev(mask, "mask", F32), float(s), float(dsigma), float(sigma_next), n, mask.numel(), _stream())
    elif v_text is not None:
        native.call("rt_cfg_euler_step_f32", x, _dev(v, "v_uncond", BF16), _dev(v_text, "v_text", BF16), xb, float(s), float(dsigma), n, _stream())
    else:
        native.call("rt_euler_step_f32", x, _dev(v, "v", BF16), xb, float(dsigma), n, _stream())
    return x32


@dataclass(frozen=True)
class StochasticArgs:
    """What the stochastic form of the master step takes besides the step's own arguments (rt_stochastic_step_f32): ``rng`` int64
    [B, 2] on the state's device, (seed, subsequence) per sample — None is allowed where sigma_next is 0, the kernel then draws
    nothing; ``sigma`` the step's sigma, ``eta`` in (0, 1] and ``sqrt_1m_eta2`` = sqrt(1 − eta²) formed by the caller in double,
    ``step`` the absolute step index (the Philox counter's third word)."""
    rng: Optional[torch.Tensor]
    sigma: float
    eta: float
    sqrt_1m_eta2: float
    step: int

    def scalars(self, sigma_next: float) -> tuple:
        return float(self.sigma), float(sigma_next), float(self.eta), float(self.sqrt_1m_eta2), int(self.step)


def _stochastic_batch(name: str, x32: torch.Tensor, st: StochasticArgs, sigma_next: float) -> Tuple[int, int]:
    """(B, n_s) of a state whose leading dimension is the batch, after the checks of ``st``."""
    if x32.dim() < 2 or x32.numel() < 1:
        raise ValueError(f"{name}: the stochastic step needs a leading batch dimension and at least one element, got shape {tuple(x32.shape)}")
    if not 0.0 < float(st.eta) <= 1.0:
        raise ValueError(f"{name}: eta must lie in (0, 1], got {st.eta}")
    if int(st.step) < 0:
        raise ValueError(f"{name}: step must not be negative, got {st.step}")
    B = x32.shape[0]
    if st.rng is None:
        if float(sigma_next) != 0.0:
            raise ValueError(f"{name}: rng is needed unless sigma_next is 0")
    elif st.rng.dtype != torch.int64 or tuple(st.rng.shape) != (B, 2) or not st.rng.is_contiguous() or st.rng.device != x32.device:
        raise ValueError(f"{name}: rng must be a contiguous int64 [{B}, 2] tensor on the state's device, got {tuple(st.rng.shape)} {st.rng.dtype}")
    return B, x32.numel() // B


def normal_fill_f32(rng: torch.Tensor, n_s: int, step: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [B, n_s]: the standard normals the stochastic step draws at ``step`` for samples whose (seed, subsequence) are the rows of
    ``rng`` (int64 [B, 2], on the GPU) — rt_normal_fill_f32, the same bits. ``out``: written in place (any shape of B·n_s elements)."""
    if rng.dtype != torch.int64 or rng.dim() != 2 or rng.shape[1] != 2 or not rng.is_contiguous():
        raise ValueError(f"normal_fill_f32: rng must be a contiguous int64 [B, 2] tensor, got {tuple(rng.shape)} {rng.dtype}")
    B = rng.shape[0]
    if out is None:
        out = torch.empty(B, int(n_s), device=rng.device, dtype=F32)
    elif out.dtype != F32 or out.numel() != B * int(n_s) or not out.is_contiguous() or out.device != rng.device:
        raise ValueError("normal_fill_f32: out must be a contiguous fp32 tensor of B·n_s elements on rng's device")
    native.call("rt_normal_fill_f32", _dev(out, "out", F32), _dev(rng, "rng", torch.int64), B, int(n_s), int(step), _stream())
    return out


def stochastic_step_f32_(x32: torch.Tensor, v: torch.Tensor, stochastic: StochasticArgs, sigma_next: float,
                         x_bf16: Optional[torch.Tensor] = None, *, v_text: Optional[torch.Tensor] = None, s: float = 0.0,
                         src32: Optional[torch.Tensor] = None, noise32: Optional[torch.Tensor] = None,
                         mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The stochastic form of the fp32 master step: x0 = x32 − sigma·vel re-noised to sigma_next with noise drawn inside the kernel,
    x32 = (1 − sigma_next)·x0 + sigma_next·n, n = z at eta = 1 and sqrt(1 − eta²)·(x0 + vel) + eta·z below; vel, the blend under
    ``mask`` and the bf16 copy as in the steps above. x32's leading dimension is the batch."""
    return _master_step_f32("stochastic_step_f32_", x32, v, v_text, s, 0.0, x_bf16, sigma_next, src32, noise32, mask, stochastic=stochastic)


def euler_step_f32_(x32: torch.Tensor, v: torch.Tensor, dsigma: float, x_bf16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x32 += dsigma*v on an fp32 master state; optionally refreshes its bf16 copy."""
    return _master_step_f32("euler_step_f32_", x32, v, None, 0.0, dsigma, x_bf16)


def cfg_euler_step_f32_(x32: torch.Tensor, v_uncond: torch.Tensor, v_text: torch.Tensor, s: float, dsigma: float,
                       x_bf16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x32 += dsigma*(u + s*(t - u)) on an fp32 master state, the mix kept in fp32; optionally refreshes its bf16 copy."""
    return _master_step_f32("cfg_euler_step_f32_", x32, v_uncond, v_text, s, dsigma, x_bf16)


def repaint_euler_step_f32_(x32: torch.Tensor, v: torch.Tensor, v_text: Optional[torch.Tensor], s: float, dsigma: float, sigma_next: float,
                           src32: torch.Tensor, noise32: torch.Tensor, mask: torch.Tensor, x_bf16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fp32 master step (``v_text`` given: the true-CFG one, ``v`` its unconditional half) followed by the latent blend of a
    repaint: x32 = (1 − m)·((1 − sigma_next)·src + sigma_next·noise) + m·(x32 + dsigma·vel); optionally refreshes the bf16 copy.
    ``mask`` has x32's shape, or a leading 1 where x32 has its batch: one mask for every sample."""
    return _master_step_f32("repaint_euler_step_f32_", x32, v, v_text, s, dsigma, x_bf16, sigma_next, src32, noise32, mask)


def multistep_step_f32_(x32: torch.Tensor, v: torch.Tensor, hist32: torch.Tensor, w: float, dsigma: float,
                        x_bf16: Optional[torch.Tensor] = None, *, v_text: Optional[torch.Tensor] = None, s: float = 0.0, sigma_next: float = 0.0,
                        src32: Optional[torch.Tensor] = None, noise32: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The second-order multistep form of the fp32 master step: x32 += dsigma·(vel + w·(vel − hist32)) and hist32 = vel, with vel, the
    blend under ``mask`` and the bf16 copy as in the three steps above. ``w`` = 0: hist32 is written and not read (it may be
    uninitialised) and x32 gets the bits of the step above that the other arguments select."""
    return _master_step_f32("multistep_step_f32_", x32, v, v_text, s, dsigma, x_bf16, sigma_next, src32, noise32, mask, hist32, w)


def guidance_partials_shape(B: int, n_s: int) -> Tuple[int, int, int]:
    """Shape of the fp32 workspace of the projected step for a state of B samples of n_s elements (rt_guidance_ws_bytes(B, n_s) bytes)."""
    return int(B), -(-int(n_s) // native.RT_GUIDE_CHUNK), 3


def projected_step_f32_(x32: torch.Tensor, v_uncond: torch.Tensor, v_text: torch.Tensor, diff32: torch.Tensor, partials: torch.Tensor, s: float,
                        eta: float, norm_threshold: float, beta: float, dsigma: float, x_bf16: Optional[torch.Tensor] = None, *,
                        hist32: Optional[torch.Tensor] = None, w: float = 0.0, sigma_next: float = 0.0, src32: Optional[torch.Tensor] = None,
                        noise32: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                        stochastic: Optional[StochasticArgs] = None) -> torch.Tensor:
    """The fp32 master step with projected guidance (guidance.py), two launches: rt_guidance_reduce_f32 — diff32 = (v_text − v_uncond)
    + beta·diff32 in fp32 and, per sample and chunk, the partial sums of (d², d·p, p²) in a fixed order — then the step with
    vel = p + (s − 1)·(k·d + e·p) in the mixed velocity's place — the multistep part (``hist32``, ``w``), the blend under ``mask`` and
    the bf16 copy as in the other steps. ``diff32`` (fp32, x32's shape) and ``partials`` are the caller's; ``beta`` is the momentum, 0
    for the first guided step of a run: diff32 is then written and not read, it may be uninitialised. x32's leading dimension is the
    batch: the sums are per sample. ``stochastic``: the stochastic rule in the Euler rule's place (rt_projected_stochastic_step_f32; no
    history, ``dsigma`` unused)."""
    name = "projected_step_f32_"
    if x32.dim() < 2 or x32.numel() < 1:
        raise ValueError(f"{name}: the state needs a leading batch dimension and at least one element, got shape {tuple(x32.shape)}")
    _check_master_step(name, x32, (v_uncond, v_text, diff32, hist32), x_bf16, src32, noise32, mask, contiguous=(partials,))
    B, n_s = x32.shape[0], x32.numel() // x32.shape[0]
    if tuple(partials.shape) != guidance_partials_shape(B, n_s):
        raise ValueError(f"{name}: partials must be {guidance_partials_shape(B, n_s)} (guidance_partials_shape), got {tuple(partials.shape)}")
    if stochastic is not None:
        if hist32 is not None:
            raise ValueError(f"{name}: the stochastic step keeps no history (solver order 1 only)")
        _stochastic_batch(name, x32, stochastic, sigma_next)
    x, xb = _dev(x32, "x32", F32), _opt(x_bf16, "x_bf16", BF16)
    pu, pt, pd, pp = _dev(v_uncond, "v_uncond", BF16), _dev(v_text, "v_text", BF16), _dev(diff32, "diff32", F32), _dev(partials, "partials", F32)
    rest = (_opt(hist32, "hist32", F32), float(w), _opt(src32 if mask is not None else None, "src32", F32),
            _opt(noise32 if mask is not None else None, "noise32", F32), _opt(mask, "mask", F32))
    native.call("rt_guidance_reduce_f32", pu, pt, pd, float(beta), pp, B, n_s, _stream())
    if stochastic is not None:
        native.call("rt_projected_stochastic_step_f32", x, pu, pt, xb, pd, pp, float(s) - 1.0, float(eta), float(norm_threshold), *rest[2:],
                    _opt(stochastic.rng, "rng", torch.int64), *stochastic.scalars(sigma_next), B, n_s,
                    x32.numel() if mask is None else mask.numel(), _stream())
        return x32
    native.call("rt_projected_step_f32", x, pu, pt, xb, pd, pp, float(s) - 1.0, float(eta), float(norm_threshold), *rest, float(dsigma),
                float(sigma_next), B, n_s, x32.numel() if mask is None else mask.numel(), _stream())
    return x32


def cfg_mix(v_uncond: torch.Tensor, v_text: torch.Tensor, s: float) -> torch.Tensor:
    u, t = v_uncond.contiguous(), v_text.contiguous()
    out = torch.empty_like(t)
    native.call("rt_cfg_mix", _dev(u, "u", BF16), _dev(t, "t", BF16), out.data_ptr(), float(s), out.numel(), _stream())
    return out


def pack_latents(x: torch.Tensor) -> torch.Tensor:
    B, Cc, H2, W2 = x.shape
    x = x.contiguous()
    out = torch.empty(B, (H2 // 2) * (W2 // 2), Cc * 4, device=x.device, dtype=BF16)
    native.call("rt_pack_latents", _dev(x, "x", BF16), out.data_ptr(), B, Cc, H2, W2, _stream())
    return out


def unpack_latents_nhwc(packed: torch.Tensor, H2: int, W2: int, scaling: float, shift: float) -> torch.Tensor:
    """[B,(H2/2)(W2/2),4C] -> NHWC [B,H2,W2,C] bf16 holding packed/scaling + shift."""
    B, _, C4 = packed.shape
    Cc = C4 // 4
    packed = packed.contiguous()
    out = torch.empty(B, H2, W2, Cc, device=packed.device, dtype=BF16)
    native.call("rt_unpack_latents", _dev(packed, "packed", BF16), out.data_ptr(), B, Cc, H2, W2, 1.0 / float(scaling), float(shift), _stream())
    return out


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=BF16)
    native.call("rt_cast_f32_to_bf16", _dev(x, "x", F32), out.data_ptr(), x.numel(), _stream())
    return out


def to_f32(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=F32)
    native.call("rt_cast_bf16_to_f32", _dev(x, "x", BF16), out.data_ptr(), x.numel(), _stream())
    return out


def masked_accumulate_(y: torch.Tensor, x: torch.Tensor, rowscale: Optional[torch.Tensor], alpha: float = 1.0, accumulate: bool = True) -> torch.Tensor:
    """y[b,r,:] (+)= alpha*rowscale[r]*x[b,r,:]; contiguous [B,R,D]; x bf16, y bf16 or f32."""
    if x.shape != y.shape or x.dim() != 3 or not x.is_contiguous() or not y.is_contiguous() or y.dtype not in (BF16, F32):
        raise ValueError("masked_accumulate_: contiguous [B,R,D] tensors of equal shape (y bf16 or f32)")
    B, R, D = x.shape
    if rowscale is not None and (rowscale.numel() != R or not rowscale.is_contiguous()):
        raise ValueError("rowscale must be contiguous with R elements")
    native.call("rt_masked_accumulate", _dev(x, "x", BF16), _dev(y, "y"), _opt(rowscale, "rowscale", F32), float(alpha), B, R, D, int(accumulate),
        int(y.dtype == F32), _stream())
    return y


def silu_split(x: torch.Tensor, apply_silu: bool = True):
    """(hi, lo) bf16 with hi + lo ~= silu(x) to ~2^-17 relative: A operands for a two-pass bf16 GEMM on fp32 activations."""
    x = x.contiguous()
    hi = torch.empty(x.shape, device=x.device, dtype=BF16)
    lo = torch.empty(x.shape, device=x.device, dtype=BF16)
    native.call("rt_silu_split_bf16", _dev(x, "x", F32), hi.data_ptr(), lo.data_ptr(), x.numel(), int(apply_silu), _stream())
    return hi, lo


def resize2d(x: torch.Tensor, size=None, scale_factor: Optional[float] = None, mode: str = "nearest", u8_scale: Optional[float] = None) -> torch.Tensor:
    """torch.nn.functional.interpolate(x, size=/scale_factor=, mode="nearest"|"bilinear", align_corners=False) on the device,
    bit-identical to ATen: x [..., H, W] fp32 — or uint8 with ``u8_scale`` (x / u8_scale is resized) — -> fp32 [..., OH, OW]."""
    if mode not in ("nearest", "bilinear"):
        raise ValueError("resize2d: mode must be 'nearest' or 'bilinear'")
    if (size is None) == (scale_factor is None):
        raise ValueError("resize2d: exactly one of size / scale_factor")
    x = x.contiguous()
    H, W = x.shape[-2], x.shape[-1]
    if size is not None:
        OH, OW = int(size[0]), int(size[1])
        sf = 0.0
    else:
        OH, OW = int(H * float(scale_factor)), int(W * float(scale_factor))   # floor(in * scale), as torch computes the size
        sf = float(scale_factor)
    is_u8 = x.dtype == torch.uint8
    if is_u8 != (u8_scale is not None) or (not is_u8 and x.dtype != F32):
        raise TypeError("resize2d: fp32 input, or uint8 input together with u8_scale")
    planes = x.numel() // (H * W)
    out = torch.empty(*x.shape[:-2], OH, OW, device=x.device, dtype=F32)
    native.call("rt_resize2d", _dev(x, "x"), int(is_u8), float(u8_scale or 1.0), out.data_ptr(), planes, H, W, OH, OW,
                                                      sf, sf, int(mode == "bilinear"), _stream())
    return out


def glyph_blend(image: torch.Tensor, latents: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """where(bilinear-resized (image > 0).any(channel) > 0, 0.10 * latents + noise, noise) — PIPE:645-654; all fp32, on the device."""
    image, latents, noise = image.contiguous(), latents.contiguous(), noise.contiguous()
    if image.dim() != 4 or latents.shape != noise.shape or latents.dim() != 4 or image.shape[0] != latents.shape[0]:
        raise ValueError("glyph_blend: image [B,C,H,W], latents/noise [B,Cl,OH,OW]")
    B, Cimg, H, W = image.shape
    _, Cl, OH, OW = latents.shape
    out = torch.empty_like(noise)
    native.call("rt_glyph_blend", _dev(image, "image", F32), _dev(latents, "latents", F32), _dev(noise, "noise", F32),
                                                             out.data_ptr(), B, Cimg, H, W, Cl, OH, OW, _stream())
    return out


def canny_u8(img: torch.Tensor, low: float = 50.0, high: float = 100.0, invert: bool = False, out_channels: int = 1) -> torch.Tensor:
    """cv2.Canny(img, low, high) of infer.py:16-22 on the device: img uint8 [H,W] or [H,W,C] -> uint8 [H,W,out_channels] edge map
    {0,255} (255 - edges with ``invert``), bit-identical to hints.canny_edges. One call = four kernels, no host sync."""
    if img.dtype != torch.uint8 or img.dim() not in (2, 3):
        raise TypeError("canny_u8: uint8 [H,W] or [H,W,C]")
    img = img.contiguous()
    H, W = img.shape[0], img.shape[1]
    Cc = 1 if img.dim() == 2 else img.shape[2]
    ws = torch.empty(int(native.load().rt_canny_ws_bytes(H, W)), device=img.device, dtype=torch.uint8)
    out = torch.empty(H, W, out_channels, device=img.device, dtype=torch.uint8)
    native.call("rt_canny_u8", _dev(img, "img"), H, W, Cc, float(low), float(high), out.data_ptr(), out_channels, int(invert),
                                               ws.data_ptr(), ws.numel(), _stream())
    return out


def preprocess_u8(img: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """VaeImageProcessor.preprocess for uint8 images already at the target size: [B,H,W,C] (or [H,W,C] / [H,W]) -> f32 [B,C,H,W]
    = x/255 (then 2x-1), bit-identical to the host path."""
    if img.dtype != torch.uint8:
        raise TypeError("preprocess_u8: uint8 input")
    if img.dim() == 2:
        img = img[None, :, :, None]
    elif img.dim() == 3:
        img = img[None]
    img = img.contiguous()
    B, H, W, Cc = img.shape
    out = torch.empty(B, Cc, H, W, device=img.device, dtype=F32)
    native.call("rt_preprocess_u8", _dev(img, "img"), out.data_ptr(), B, H, W, Cc, int(normalize), _stream())
    return out


def _window(window, H: int, W: int, name: str):
    """(x0, y0, cw, ch) of a crop rectangle inside an H x W image."""
    x0, y0, cw, ch = (int(v) for v in window)
    if cw < 1 or ch < 1 or x0 < 0 or y0 < 0 or x0 + cw > W or y0 + ch > H:
        raise ValueError(f"{name}: window (x0={x0}, y0={y0}, w={cw}, h={ch}) is not inside the {W}x{H} image")
    return x0, y0, cw, ch


def resize_aa(x: torch.Tensor, window, size, mul: float = 1.0, add: float = 0.0) -> torch.Tensor:
    """Crop + antialiased bilinear resample on the device: the ``window`` (x0, y0, w, h; None: all of it) of ``x`` — uint8 [H,W] / [H,W,C]
    interleaved (a sample is x/255) or fp32 [C,H,W] planar, C in {1, 3} — to fp32 [C, size[0], size[1]] = mul·r + add. The filter is
    ``F.interpolate(window, size, mode="bilinear", antialias=True, align_corners=False)``; a window resampled to its own size is
    mul·(x/255) + add bit for bit. At most native.RT_RESIZE_AA_MAX_SCALE input samples per output sample and axis."""
    is_u8 = x.dtype == torch.uint8
    if not ((is_u8 and x.dim() in (2, 3)) or (x.dtype == F32 and x.dim() == 3)):
        raise TypeError("resize_aa: uint8 [H,W] / [H,W,C] or fp32 [C,H,W]")
    x = x.contiguous()
    if is_u8:
        H, W, Cc = x.shape[0], x.shape[1], (1 if x.dim() == 2 else x.shape[2])
    else:
        Cc, H, W = x.shape
    x0, y0, cw, ch = _window((0, 0, W, H) if window is None else window, H, W, "resize_aa")
    OH, OW = int(size[0]), int(size[1])
    if OH < 1 or OW < 1:
        raise ValueError(f"resize_aa: size {tuple(size)}")
    out = torch.empty(Cc, OH, OW, device=x.device, dtype=F32)
    ws = torch.empty(int(native.load().rt_resize_aa_ws_bytes(Cc, ch, OW)), device=x.device, dtype=torch.uint8)
    native.call("rt_resize_aa", _dev(x, "x"), int(is_u8), Cc, H, W, x0, y0, cw, ch, out.data_ptr(), OH, OW, float(mul), float(add),
                ws.data_ptr(), ws.numel(), _stream())
    return out


def gaussian_blur(plane: torch.Tensor, sigma: float) -> torch.Tensor:
    """Separable Gaussian blur of one fp32 plane [H,W]: radius ceil(3·sigma), fp32 weights normalised to sum 1, replicated borders.
    sigma = 0 returns the plane; sigma above native.RT_BLUR_MAX_RADIUS / 3 is refused."""
    if plane.dim() != 2:
        raise ValueError(f"gaussian_blur: one [H,W] plane, got {tuple(plane.shape)}")
    _dev(plane, "plane", F32)
    if float(sigma) < 0:
        raise ValueError(f"gaussian_blur: sigma {sigma} < 0")
    if float(sigma) == 0:
        return plane
    plane = plane.contiguous()
    H, W = plane.shape
    out, ws = torch.empty_like(plane), torch.empty_like(plane)
    native.call("rt_gaussian_blur_f32", plane.data_ptr(), out.data_ptr(), H, W, float(sigma), ws.data_ptr(), ws.numel() * 4, _stream())
    return out


def composite_u8(photo: torch.Tensor, gen: torch.Tensor, alpha: torch.Tensor, window) -> torch.Tensor:
    """A copy of ``photo`` (uint8 [H,W,C], C in {1, 3}) with ``gen`` (fp32 [C,h,w] in [-1,1], the decoder's range) blended into the
    ``window`` (x0, y0, w, h) under ``alpha`` (fp32 [h,w] in [0,1]): rint((1 − a)·photo + a·clamp(gen/2 + 0.5, 0, 1)·255). alpha 0 keeps
    the photo's byte, alpha 1 writes the byte the decoder's uint8 output has for ``gen``."""
    if photo.dtype != torch.uint8 or photo.dim() != 3:
        raise TypeError("composite_u8: photo uint8 [H,W,C]")
    photo, gen, alpha = photo.contiguous(), gen.contiguous(), alpha.contiguous()
    H, W, Cc = photo.shape
    x0, y0, cw, ch = _window(window, H, W, "composite_u8")
    if tuple(gen.shape) != (Cc, ch, cw) or tuple(alpha.shape) != (ch, cw):
        raise ValueError(f"composite_u8: gen {tuple(gen.shape)} / alpha {tuple(alpha.shape)} against a {cw}x{ch} window of {Cc} channels")
    out = torch.empty_like(photo)
    native.call("rt_composite_u8", _dev(photo, "photo"), out.data_ptr(), H, W, Cc, x0, y0, cw, ch, _dev(gen, "gen", F32), _dev(alpha, "alpha", F32),
                _stream())
    return out
