"""The kernels that produce e4m3 operands — rt_quantize_rows_fp8, rt_layernorm_modulate_fp8, rt_attention_fp8_prep — and the e4m3
attention that consumes them (rt_attention_fp8_fwd, rt_attention_fp8_fwd_mx) at the lengths where a flash kernel goes wrong, against fp64
references computed on the CPU from exactly the values the kernel reads, judged PER ELEMENT (support_kernels.check_bound) wherever the
arithmetic allows it.

Every case works on views of larger buffers: a row stride greater than the width and a padded batch stride, NaN (0x7f bytes for e4m3)
where the kernel must not read or has to write, a sentinel around what it writes, everything outside compared bit for bit afterwards.
Every launch runs twice from restored buffers and must repeat its bits. Each case prints its worst err/bound and where (run with -s).

Dispatch reached (csrc/norm_elem.hip; nch = ceil(D / 512)):
    rt_quantize_rows_fp8, bf16 x: D = 8, 3072 -> quantize_rows_fp8_kernel<false, 6>; 3080, 6144 -> <false, 12>; 6152, 12288 -> <false, 24>;
        12296, 15360 -> <false, 30>; 15368, 65536 -> quantize_rows_fp8_kernel<false, 0> (two passes). fp32 x: quantize_rows_fp8_kernel<true, 0>.
    rt_layernorm_modulate_fp8: D = 8, 1024 -> layernorm_mod_kernel<., 2, true>; 1032, 3072 -> <., 6, true>; 3080, 8192 -> <., 16, true>;
        bf16 and fp32 x each."""
import math

import pytest
import torch

from support_kernels import (BF16, F32, FP8, NAN, NAN_U8, QK_COUNTED, QK_EPS, SENT, U23, check_bound, check_quant_rows, e4m3_finite, fold_zero,
                             guarded3, layernorm_ref, ln_case, outside3_is, qk_layout, qk_norm_rope_ref, qk_tables, qk_weights,
                             quant_rows_rule, rel_l2, same_bits, twice, ulp_e4m3, vt8_expected)

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402

ids_dt = lambda dt: "bf16" if dt == BF16 else "f32"


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


def e4m3_out(B, R, D, gpu):
    """uint8 [B, R + 2, D + 16] holding 0x7f (a byte the kernel fails to write is a NaN operand later), and its [B, R, D] e4m3 view."""
    buf = torch.full((B, R + 2, D + 16), NAN_U8, dtype=torch.uint8, device=gpu)
    return buf, buf.view(FP8)[:, :R, :D]


def scale_out(n, gpu):
    """fp32 [n + 8] holding the sentinel, and its contiguous [n] slice four floats in."""
    buf = torch.full((n + 8,), SENT, dtype=F32, device=gpu)
    return buf, buf[4 : 4 + n]


def scale_guards_intact(buf, n):
    return same_bits(buf[:4], torch.full_like(buf[:4], SENT)) and same_bits(buf[4 + n :], torch.full_like(buf[4 + n :], SENT))


# ------------------------------------------------------------------------------------------------ row quantisation
QR_B, QR_R = 2, 5
QR_D = [(D, BF16) for D in (8, 3072, 3080, 6144, 6152, 12288, 12296, 15360, 15368, 65536)] + [(D, F32) for D in (8, 520, 3072)]


def quant_case(D, dtype, seed):
    """x [QR_B, 5, D] in `dtype` on the CPU, row magnitudes 1e-3 .. 1e2: row 0 all zero (scale 1.0, zero bytes); row 1 with a
    negative maximum in the last 8 columns; row 2 with its maximum in the first 8 columns of the last 512-column chunk (where a
    chunk dropped from the max pass shows); row 3 with the maximum exactly 448 x 2^3; row 4 plain."""
    g = torch.Generator().manual_seed(seed)
    mags = torch.logspace(-3, 2, QR_R)
    x = torch.randn(QR_B, QR_R, D, generator=g) * mags[None, :, None]
    for b in range(QR_B):
        x[b, 0] = 0
        x[b, 1, D - 2 - b] = -2.0 * float(x[b, 1].abs().max())
        x[b, 2, (D - 1) // 512 * 512 + 3 + b] = 2.0 * float(x[b, 2].abs().max())
        x[b, 3] = x[b, 3].clamp(-3000.0, 3000.0)
        x[b, 3, D // 2] = 448.0 * 8
    return x.to(dtype)


@pytest.mark.parametrize("D,dtype", QR_D, ids=[f"{D}-{ids_dt(dt)}" for D, dt in QR_D])
def test_quantize_rows_per_element(ops, gpu, D, dtype):
    """ops.quantize_rows_fp8_into on a [2, 5, D] view (ld = D + 8, two NaN rows behind every batch entry), and ops.quantize_rows_fp8
    on its first batch entry (same bits). Checks, per row and per element:
      scale == fp32(amax * fp32(1 / 448)) bit for bit, 1.0 for the all-zero row, whose bytes are zero;
      every byte finite; |q - t| <= ulp_e4m3(t) / 2 + 2^-21 |t| with t = x / scale_got in fp64 (support_kernels.check_quant_rows:
        the rounding to the e4m3 grid; the fp32 reciprocal and product, three roundings, one possibly a whole ulp);
      fewer than 1e-3 of the bytes differ from round-to-nearest-even of the same fp32 arithmetic on the CPU (quant_rows_rule);
      0x7f outside the output view, the sentinel around the scales, the input unchanged."""
    x = quant_case(D, dtype, seed=D)
    xbuf, xv = guarded3(x, 2, D + 8, NAN, dtype, gpu)

    def run():
        obuf, out = e4m3_out(QR_B, QR_R, D, gpu)
        sbuf, sc = scale_out(QR_B * QR_R, gpu)
        ops.quantize_rows_fp8_into(xv, out, sc)
        return obuf, sbuf

    obuf, sbuf = twice(run)
    q = obuf.view(FP8)[:, :QR_R, :D].cpu().reshape(QR_B * QR_R, D)
    sc = sbuf[4 : 4 + QR_B * QR_R].cpu()
    rows = x.reshape(QR_B * QR_R, D)
    q_rule, sc_rule = quant_rows_rule(rows)
    assert same_bits(sc, sc_rule), (sc, sc_rule)
    assert float(sc[0]) == 1.0 and not bool(fold_zero(q[0]).any()) and float(sc[3]) == 8.0
    check_quant_rows(f"quantize_rows D={D} {ids_dt(dtype)}", q, sc, rows)
    mism = float((fold_zero(q) != fold_zero(q_rule)).float().mean())
    print(f"[bytes] quantize_rows D={D} {ids_dt(dtype)}: {mism:.2e} of the bytes differ from the CPU's round-to-nearest-even")
    assert mism < 1e-3
    assert outside3_is(obuf, QR_R, D, NAN_U8) and scale_guards_intact(sbuf, QR_B * QR_R), "wrote outside its views"
    assert same_bits(xbuf.cpu(), guarded3(x, 2, D + 8, NAN, dtype)[0]), "the input changed"
    q0, s0 = ops.quantize_rows_fp8(xv[0])
    assert same_bits(q0.cpu().view(torch.uint8), q[:QR_R].view(torch.uint8)) and same_bits(s0.cpu(), sc[:QR_R])


# ------------------------------------------------------------------------------------------------ LayerNorm -> e4m3
LN_B, LN_R = 2, 5


@pytest.mark.parametrize("xdtype", [BF16, F32], ids=ids_dt)
@pytest.mark.parametrize("D", [8, 1024, 1032, 3072, 3080, 8192])
def test_layernorm_modulate_fp8_per_element(ops, gpu, D, xdtype):
    """ops.layernorm_modulate_fp8 on the data and views of test_token_passes_gpu.test_layernorm_modulate_per_element. y, by = the fp64
    reference and its fp32-evaluation bound (support_kernels.layernorm_ref, without the bf16 term: nothing is rounded to bf16 here).
      |row_scale - max|y| / 448| <= by(at the argmax) / 448 + 2^-22 row_scale       (the product with fp32(1 / 448): two roundings)
      |q row_scale_got - y| <= ulp_e4m3(y / row_scale_got) / 2 x row_scale_got + by + 2^-21 |y|
    the rounding to the e4m3 grid, the evaluation of y, the fp32 reciprocal and product. Every byte finite; 0x7f around out, the
    sentinel around row_scale; fewer than 2 % of the bytes differ from the CPU emulation (fp32 LayerNorm, then quant_rows_rule)."""
    x, table, shift, scale = ln_case(LN_B, LN_R, D, xdtype, seed=D)
    _, xv = guarded3(x, 2, D + 8, NAN, xdtype, gpu)
    tab = table.to(gpu)
    n = LN_B * LN_R

    def run():
        obuf, out = e4m3_out(LN_B, LN_R, D, gpu)
        sbuf, rs = scale_out(n, gpu)
        ops.layernorm_modulate_fp8(xv, out, rs, tab[:, 4 : 4 + D], tab[:, 4 + D : 4 + 2 * D])
        return obuf, sbuf

    obuf, sbuf = twice(run)
    what = f"layernorm_fp8 D={D} {ids_dt(xdtype)}"
    q = obuf.view(FP8)[:, :LN_R, :D].cpu()
    rs = sbuf[4 : 4 + n].cpu().double().reshape(LN_B, LN_R, 1)
    assert e4m3_finite(q), "NaN byte"
    y, by = layernorm_ref(x, shift, scale)
    am = y.abs().argmax(dim=-1, keepdim=True)
    check_bound(f"{what} row_scale", rs, y.abs().gather(-1, am) / 448.0, by.gather(-1, am) / 448.0 + 2.0 ** -22 * rs)
    check_bound(f"{what} q x row_scale", q.float().double() * rs, y, 0.5 * ulp_e4m3(y / rs) * rs + by + 2.0 ** -21 * y.abs())
    y32 = orc.layer_norm(x.float()) * (1 + scale[:, None]) + shift[:, None]
    q_rule, _ = quant_rows_rule(y32.reshape(n, D))
    mism = float((fold_zero(q.reshape(n, D)) != fold_zero(q_rule)).float().mean())
    print(f"[bytes] {what}: {mism:.2e} of the bytes differ from the CPU emulation")
    assert mism < 2e-2
    assert outside3_is(obuf, LN_R, D, NAN_U8) and scale_guards_intact(sbuf, n), "wrote outside its views"


# ------------------------------------------------------------------------------------------------ e4m3 attention operands
# The excess of |q - t| over ulp_e4m3(t) / 2 + 16 QK_COUNTED 2^-23 (|a cos| + |b sin|), relative to 16 (|a cos| + |b sin|): what the
# device rsqrtf adds to the counted roundings of prep_qk_kernel (the arithmetic of rt_qk_norm_rope8, contracted as the compiler likes).
# Measured on an MI355X over every case of test_attention_fp8_prep_per_element (each prints its own; run with -s):
MEASURED_PREP_RSQRT_EXCESS = 0.0    # MI355X: nothing above the counted terms in any case (largest (1, 129, 40, 3)); counted terms alone
PREP_SHAPES = [(1, 1, 0, 1, False), (2, 63, 20, 2, False), (2, 64, 64, 2, False), (2, 65, 0, 2, False), (1, 129, 40, 3, False),
               (2, 63, 20, 2, True)]


class PrepCase:
    """One rt_attention_fp8_prep launch on guarded buffers. The fused projection buffer is [B, S + 2, ld] bf16 with NaN in the rows
    behind S, in the pad columns and (single-block layout: k at 0, v at d, q at 2 d, ld = 7 d + 8) in the mlp columns; the double-block
    layout is q | k | v with ld = 3 d + 8. qk8 and vt8 are the heads of byte buffers holding 0x7f, 64 bytes longer than needed.
    hard: the far-apart norm weights of the q/k pass's tests with weight 3 at element 5, a one-hot q head (16 n > 448) at (0, 0, head
    0), v with values that saturate (+-1000, 464, 480) and the key index pattern v[j][0] = j % 16 - 8 in channel 0; otherwise weights
    1 + 0.1 randn and plain N(0, 1) operands, as test_kernels_gpu.test_attention_fp8 has them."""

    def __init__(self, ops, gpu, B, S, T, H, single=False, hard=True, seed=0):
        from reptext_amd import native

        self.B, self.S, self.T, self.H, self.d = B, S, T, H, H * 128
        d = self.d
        g = torch.Generator().manual_seed(seed + 31 * S + H)
        self.q_off, self.k_off, ld = qk_layout(single, d)
        self.v_off = d if single else 2 * d
        q, k, v = (torch.randn(B, S, d, generator=g).to(BF16) for _ in range(3))
        if hard:
            self.w = qk_weights(S)
            self.w[0][5] = self.w[2][5] = 3.0
            q[0, 0, :128] = 0
            q[0, 0, 5] = 2.0
            for i, val in enumerate((1000.0, -1000.0, 464.0, 480.0, -464.0)):
                v[(i + 1) % B, (7 * i + 3) % S, 11 * i + 1] = val
            v[:, :, 0] = ((torch.arange(S) % 16) - 8).to(BF16)[None, :]
        else:
            self.w = [(1.0 + 0.1 * torch.randn(128, generator=g)).to(BF16) for _ in range(4)]
        self.q, self.k, self.v = q, k, v
        self.cos, self.sin = qk_tables(S, T)
        host = torch.full((B, S + 2, ld), NAN, dtype=BF16)
        for off, t in ((self.q_off, q), (self.k_off, k), (self.v_off, v)):
            host[:, :S, off : off + d] = t
        self.host, self.buf = host, host.to(gpu)
        self.vt_bytes = int(native.load().rt_attention_fp8_vt_bytes(B, S, H))
        self.qk_bytes = B * S * 2 * d
        self.qk_big = torch.full((self.qk_bytes + 64,), NAN_U8, dtype=torch.uint8, device=gpu)
        self.vt_big = torch.full((self.vt_bytes + 64,), NAN_U8, dtype=torch.uint8, device=gpu)
        self.qk8 = self.qk_big[: self.qk_bytes].view(FP8).view(B, S, 2 * d)
        self.vt8 = self.vt_big[: self.vt_bytes].view(FP8)
        wd = [t.to(gpu) for t in self.w]
        ops.attention_fp8_prep(self.buf[:, :S], self.q_off, self.k_off, self.v_off, H, T, wd[0] if T > 0 else None, wd[1] if T > 0 else None,
                               wd[2], wd[3], self.cos.to(gpu), self.sin.to(gpu), self.qk8, self.vt8, eps=QK_EPS)

    def heads(self, t):
        return t.reshape(self.B, self.S, self.H, 128)

    def guards_intact(self):
        tail = torch.full((64,), NAN_U8, dtype=torch.uint8, device=self.qk_big.device)
        return same_bits(self.qk_big[self.qk_bytes :], tail) and same_bits(self.vt_big[self.vt_bytes :], tail) and \
            same_bits(self.buf.cpu(), self.host)


@pytest.mark.parametrize("B,S,T,H,single", PREP_SHAPES, ids=[f"{B}-{S}-{T}-{H}-{'single' if s else 'double'}" for B, S, T, H, s in PREP_SHAPES])
def test_attention_fp8_prep_per_element(ops, gpu, B, S, T, H, single):
    """rt_attention_fp8_prep's two outputs.
    vt8 is exact: byte [b][h][dd][64 t + p], p = 32 hh + 16 kt + 4 g + e, is e4m3(clamp(v[b][64 t + 32 kt + 8 g + 4 hh + e][h 128 + dd],
    +-448)), zero for keys >= S — built on the CPU from the layout comment at the top of csrc/attention_fp8.hip
    (support_kernels.vt8_expected) and compared as bytes, -0 folded onto +0. v holds +-1000, 464 and 480 (saturate at +-448, no NaN)
    and channel 0 holds j % 16 - 8, so a permutation error names the keys it mixed up.
    qk8: with n the fp64 normalised and rotated value (support_kernels.qk_norm_rope_ref), t = clamp(16 n, +-448),
        |q - t| <= ulp_e4m3(t) / 2 + 16 (QK_COUNTED 2^-23 + 4 MEASURED_PREP_RSQRT_EXCESS) (|a cos| + |b sin|)
    the rounding to the e4m3 grid and the fp32 evaluation as counted for the q/k pass (the x 16 is exact). q in columns [0, d), k in
    [d, 2 d). The one-hot q head with weight 3 has 16 n = 543: its byte is +448. buf is unchanged; the bytes behind both outputs
    still hold 0x7f, and none inside them does."""
    c = PrepCase(ops, gpu, B, S, T, H, single=single)
    first = (c.qk_big.clone(), c.vt_big.clone())
    c2 = PrepCase(ops, gpu, B, S, T, H, single=single)
    assert same_bits(first[0], c2.qk_big) and same_bits(first[1], c2.vt_big), "not bitwise repeatable"
    what = f"fp8_prep {'single' if single else 'double'} B={B} S={S} T={T} H={H}"
    assert c.guards_intact(), "wrote behind an output, or changed buf"
    assert e4m3_finite(c.qk8) and e4m3_finite(c.vt8), "a NaN byte inside an output"
    # vt8
    d = c.d
    got = fold_zero(c.vt8.cpu()).reshape(B, H, 128, -1)
    exp = vt8_expected(c.heads(c.v))
    bad = (got != exp).nonzero()
    print(f"[bytes] {what} vt8: {len(bad)} of {exp.numel()} bytes differ" + (f", first at [b, h, dd, pos] = {bad[0].tolist()}: channel-0 row holds "
          f"{got[bad[0][0], bad[0][1], 0].view(FP8).float().tolist()[:64]}" if len(bad) else ""))
    assert len(bad) == 0
    # qk8
    qk = c.qk8.cpu().float().double()
    for name, col, x, wt, wi in (("q", 0, c.q, c.w[0], c.w[2]), ("k", d, c.k, c.w[1], c.w[3])):
        ref, mag = qk_norm_rope_ref(c.heads(x), wt, wi, T, c.cos, c.sin, QK_EPS)
        t = (16.0 * ref).clamp(-448.0, 448.0)
        bound = 0.5 * ulp_e4m3(t) + 16.0 * (QK_COUNTED * U23 + 4 * MEASURED_PREP_RSQRT_EXCESS) * mag
        got8 = c.heads(qk[..., col : col + d])
        excess = (((got8 - t).abs() - 0.5 * ulp_e4m3(t)) / (16.0 * mag).clamp_min(1e-300) - QK_COUNTED * U23)[mag > 0]
        print(f"[rsqrt] {what} {name}8: excess over the counted terms {max(float(excess.max()), 0.0):.3e} "
              f"(MEASURED_PREP_RSQRT_EXCESS {MEASURED_PREP_RSQRT_EXCESS:.3e})")
        check_bound(f"{what} {name}8", got8, t, bound)
    assert float(qk[0, 0, 5]) == 448.0 and float(16 * qk_norm_rope_ref(c.heads(c.q), c.w[0], c.w[2], T, c.cos, c.sin, QK_EPS)[0][0, 0, 0, 5]) > 448.0


# ------------------------------------------------------------------------------------------------ e4m3 attention, length sweep
ATT_B, ATT_H = 2, 2
ATT_LENGTHS = [1, 7, 63, 64, 65, 127, 128, 129, 191]


def attn_out(B, S, d, gpu):
    """bf16 [B, S + 3, d + 8] holding the sentinel, and its [B, S, d] view."""
    buf = torch.full((B, S + 3, d + 8), SENT, dtype=BF16, device=gpu)
    return buf, buf[:, :S, :d]


def run_attention(ops, gpu, qk8, vt8, B, S, H, scale=None):
    """Twice into fresh guarded outputs, identical bits, guards intact. Returns the [B, S, d] result on the CPU."""
    def run():
        obuf, out = attn_out(B, S, H * 128, gpu)
        ops.attention_fp8(qk8, vt8, out, H, scale=scale)
        return obuf

    obuf = twice(run)
    assert outside3_is(obuf, S, H * 128, SENT), "wrote outside the output view"
    return obuf[:, :S, : H * 128].cpu()


@pytest.fixture(scope="module")
def att_cases(ops, gpu):
    """PrepCase per length, built once and shared by the tests below (which leave it unchanged)."""
    cache = {}

    def get(S):
        if S not in cache:
            cache[S] = PrepCase(ops, gpu, ATT_B, S, S // 3, ATT_H, hard=False, seed=5)
        return cache[S]

    return get


@pytest.mark.parametrize("S", ATT_LENGTHS)
def test_attention_fp8_length_sweep_exact_forms(ops, gpu, att_cases, S):
    """rt_attention_fp8_fwd at S = one ragged tile, 64 k - 1, 64 k, 64 k + 1 with operands that leave no e4m3 rounding of the numerators,
    so the verdict is per element. v8 = the e4m3 values of v, as rt_attention_fp8_prep wrote them (guarded buffers, see PrepCase).
      q = 0: every row is the mean over the S keys of v8.  |got - ref| <= 2^-8 |ref| + (S + 8) 2^-23 mean|v8|
      q = e_0, k_j = -pattern(j) e_0, scale = ln 2, pattern = j % 8, (j >> 3) % 8, (j >> 6) % 8: ref = sum_j 2^-pat(j) v8_j / sum_j 2^-pat(j),
        |got - ref| <= 2^-8 |ref| + (S + 8) 2^-23 sum_j 2^-pat(j) |v8_j| / sum_j 2^-pat(j)
    2^-8 |ref|: the bf16 rounding of the output; the rest: S fp32 accumulations and the normalisation, relative to the weighted mean
    of |v8|. Key 0 has pattern 0 in all three, so the running maximum is final after the first tile and every numerator is an exact
    power of two in e4m3's normal range. A key >= S that is not masked, a wrong clamp of the ragged tile's staging or a permuted key is
    an O(1) error at its element. The output is a [B, S, d] view of a sentinel-filled [B, S + 3, d + 8] buffer."""
    c = att_cases(S)
    B, H, d = ATT_B, ATT_H, c.d
    v8 = c.heads(c.v).float().clamp(-448.0, 448.0).to(FP8).float().double()
    qk0 = c.qk8.clone()
    qk0[..., :d] = 0
    got = run_attention(ops, gpu, qk0, c.vt8, B, S, H)
    ref = v8.mean(dim=1, keepdim=True).expand(-1, S, -1, -1).reshape(B, S, d)
    mab = v8.abs().mean(dim=1, keepdim=True).expand(-1, S, -1, -1).reshape(B, S, d)
    check_bound(f"attention_fp8 S={S} q=0", got, ref, 2.0 ** -8 * ref.abs() + (S + 8) * U23 * mab)
    j = torch.arange(S)
    for name, pat in (("low bits", j % 8), ("group / half", (j >> 3) % 8), ("tile", (j >> 6) % 8)):
        qk = torch.zeros(B, S, 2 * d)
        for hd in range(H):
            qk[:, :, hd * 128] = 16.0
            qk[:, :, d + hd * 128] = -16.0 * pat.float()
        got = run_attention(ops, gpu, qk.to(FP8).to(gpu), c.vt8, B, S, H, scale=math.log(2.0))
        wgt = torch.exp2(-pat.double())[None, :, None, None]
        ref = ((wgt * v8).sum(dim=1, keepdim=True) / wgt.sum()).expand(-1, S, -1, -1).reshape(B, S, d)
        mab = ((wgt * v8.abs()).sum(dim=1, keepdim=True) / wgt.sum()).expand(-1, S, -1, -1).reshape(B, S, d)
        check_bound(f"attention_fp8 S={S} pattern '{name}'", got, ref, 2.0 ** -8 * ref.abs() + (S + 8) * U23 * mab)
    assert c.guards_intact()


@pytest.mark.parametrize("S", ATT_LENGTHS)
def test_attention_fp8_length_sweep_random_operands(ops, gpu, att_cases, S):
    """Random operands at the same lengths, the criteria of test_kernels_gpu.test_attention_fp8: rel-L2 against the oracle's attention
    with the same static e4m3 quantisation (e8) and against its fp32 attention (e32), floor = the distance between those two:
    e32 < 1.25 floor + 2e-3 and e8 < 1.45 floor + 2e-3. And entry b of the batched launch equals the batch-1 launch of that entry,
    bit for bit."""
    c = att_cases(S)
    B, H, T, d = ATT_B, ATT_H, c.T, c.d
    q, k, v = (c.heads(t).float() for t in (c.q, c.k, c.v))
    w = [t.float() for t in c.w]

    def norm(x, wt, wi):
        y = torch.empty_like(x)
        y[:, :T] = orc.rms_norm(x[:, :T], wt)
        y[:, T:] = orc.rms_norm(x[:, T:], wi)
        return orc.apply_rope(y, c.cos, c.sin)

    qn, kn = norm(q, w[0], w[2]), norm(k, w[1], w[3])
    ref = orc.attention(qn, kn, v)
    with orc.fp8_attention():
        ref8 = orc.attention(qn, kn, v)
    got = run_attention(ops, gpu, c.qk8, c.vt8, B, S, H)
    e8, e32, floor = rel_l2(got.float(), ref8), rel_l2(got.float(), ref), rel_l2(ref8, ref)
    print(f"[attention_fp8] S={S}: {e8:.3e} vs e4m3 oracle, {e32:.3e} vs fp32 oracle (floor {floor:.3e})")
    assert e32 < 1.25 * floor + 2e-3 and e8 < 1.45 * floor + 2e-3
    per = c.vt_bytes // B
    for b in range(B):
        one = run_attention(ops, gpu, c.qk8[b : b + 1], c.vt8[b * per : (b + 1) * per], 1, S, H)
        assert same_bits(one[0], got[b]), f"batch entry {b} differs from its batch-1 launch"
    assert c.guards_intact()


@pytest.mark.parametrize("S", [1, 63, 65, 129])
def test_attention_fp8_mx_length_sweep(ops, gpu, att_cases, S):
    """rt_attention_fp8_fwd_mx at ragged lengths against the bf16-output launch of the same operands, by the rule of
    test_mx_gpu.test_attention_fp8_block_scaled_output: the de-quantised e4m3 output may differ from the bf16 one by the two roundings
    only (2^-4 + 2^-8 of the element, or half a subnormal step of its block), every scale byte is the rule applied to its block, one step
    of slack for a block maximum that the bf16 rounding moved across a boundary. The output goes into columns 256.. of rows < S of a
    zeroed [B, S + 3, 256 + d] buffer and the matching slice of a zeroed scale tensor; nothing else of either may change."""
    c = att_cases(S)
    B, H, d = ATT_B, ATT_H, c.d
    r = run_attention(ops, gpu, c.qk8, c.vt8, B, S, H).float()
    wide = 256 + d

    def run():
        big = torch.zeros(B, S + 3, wide, device=gpu, dtype=FP8)
        sc = ops.BlockScales.empty(B, S, wide, gpu)
        sc.t.fill_(0)
        ops.attention_fp8_mx(c.qk8, c.vt8, big[:, :S, 256:], sc.cols(256), H)
        return big.view(torch.uint8), sc.t

    big, sct = twice(run)
    sc = ops.BlockScales(sct, (S + 63) // 64 * 64)
    out8 = big.view(FP8)[:, :S, 256:]
    assert e4m3_finite(out8)
    deq = ops.dequantize_mx(out8.contiguous(), sc.cols(256)).cpu()
    sb = sc.cols(256).rowmajor(B, S, d).cpu().float()
    step = torch.exp2(sb - 127.0 - 10.0).repeat_interleave(32, dim=-1)
    bad = (deq - r).abs() > r.abs() * (2.0 ** -4 + 2.0 ** -8) + step
    assert not bool(bad.any()), int(bad.sum())
    rule = orc.mx_scale_byte(r.reshape(B, S, d // 32, 32).abs().amax(dim=-1)).float()
    assert bool(((sb - rule).abs() <= 1).all()) and float((sb != rule).float().mean()) < 0.02
    assert not bool(big[:, :, :256].any()) and not bool(big[:, S:].any()), "wrote outside the output slice"
    allsc = sc.rowmajor(B, sc.R, wide).clone()
    allsc[:, :S, 8 : 8 + d // 32] = 0
    assert not bool(allsc.any()), "wrote a scale byte outside the slice"
    assert c.guards_intact()
