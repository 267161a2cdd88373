"""The passes that run between the GEMMs on every block of every denoising step — rt_layernorm_modulate, rt_layernorm_modulate_pair,
rt_qk_rmsnorm_rope, rt_gemv_bf16w — against fp64 references computed on the CPU from exactly the values the kernel reads, judged PER
ELEMENT (support_kernels.check_bound), at every width where the dispatch takes another instantiation and on both sides of it.

Every case works on views of larger buffers: a row stride greater than the width and a padded batch stride, NaN where the kernel must
not read, a sentinel (or, for the in-place pass, recognisable finite values) where it must not write, and everything outside the view
compared bit for bit afterwards. Every launch runs twice from restored buffers and must repeat its bits. Each case prints its worst
err/bound and where (run with -s).

Dispatch reached (csrc/norm_elem.hip, launch_layernorm: NCH = the first of {1, 2, 4, 6, 8, 16} >= ceil(D / 512)):
    D = 8, 64, 512 -> 1;  520, 1024 -> 2;  1032, 2048 -> 4;  2056, 3072 -> 6;  3080, 4096 -> 8;  4104, 8192 -> 16; bf16 and fp32 x each.
The pair form takes the same kernels with two segments (D = 520 -> 2, 3072 -> 6)."""
import pytest
import torch

from support_kernels import (BF16, F32, NAN, QK_COUNTED, QK_EPS, SENT, U23, check_bound, guarded3, guarded_rows, layernorm_ref, ln_case,
                             outside3_is, outside_is, qk_layout, qk_norm_rope_ref, qk_tables, qk_weights, same_bits, twice)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


# ------------------------------------------------------------------------------------------------ LayerNorm + modulation
LN_D = [8, 64, 512, 520, 1024, 1032, 2048, 2056, 3072, 3080, 4096, 4104, 8192]
LN_B, LN_R = 2, 5                # ten rows: three workgroups of four waves, the last half empty
ids_dt = lambda dt: "bf16" if dt == BF16 else "f32"


def ln_bound(y, by):
    return 2.0 ** -8 * y.abs() + by


@pytest.mark.parametrize("xdtype", [BF16, F32], ids=ids_dt)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_modulate_per_element(ops, gpu, D, xdtype):
    """ops.layernorm_modulate with shift / scale and with None, None, against support_kernels.layernorm_ref. Bound per element:
        2^-8 |y| + by
    2^-8 |y|: the bf16 rounding of the output (at least half a bf16 ulp of y). by: the fp32 evaluation, every term of it named in
    layernorm_ref's docstring (row mean and variance at summation depth ln_depth(D), rsqrtf, the element's own operations).
    Rows: random, a large offset (100 + randn), constant (variance 0: the output is shift up to by, and finite), one large element
    in the last 8 columns. x is a [B, R, D] view with ld = D + 8 and two NaN rows behind every batch entry; shift and scale are chunk
    views of one NaN-padded [B, 2 D + 8] table; the output a view of a sentinel-filled [B, R + 2, D + 16] buffer."""
    x, table, shift, scale = ln_case(LN_B, LN_R, D, xdtype, seed=D)
    xbuf, xv = guarded3(x, 2, D + 8, NAN, xdtype, gpu)
    tab = table.to(gpu)
    sh, sc = tab[:, 4 : 4 + D], tab[:, 4 + D : 4 + 2 * D]
    for name, (s_d, c_d, s_h, c_h) in {"modulated": (sh, sc, shift, scale), "plain": (None, None, None, None)}.items():
        def run():
            obuf = torch.full((LN_B, LN_R + 2, D + 16), SENT, dtype=BF16, device=gpu)
            ops.layernorm_modulate(xv, obuf[:, :LN_R, :D], s_d, c_d)
            return obuf

        obuf = twice(run)
        y, by = layernorm_ref(x, s_h, c_h)
        check_bound(f"layernorm {name} D={D} {ids_dt(xdtype)}", obuf[:, :LN_R, :D], y, ln_bound(y, by))
        assert outside3_is(obuf, LN_R, D, SENT), "wrote outside the output view"
    assert same_bits(xbuf.cpu(), guarded3(x, 2, D + 8, NAN, xdtype)[0]) and same_bits(tab.cpu(), table), "an input changed"


@pytest.mark.parametrize("none_seg", [0, 1])
@pytest.mark.parametrize("xdtype", [BF16, F32], ids=ids_dt)
@pytest.mark.parametrize("D", [520, 3072])
def test_layernorm_modulate_pair_per_element(ops, gpu, D, xdtype, none_seg):
    """ops.layernorm_modulate_pair: two segments with their own (B, R) = (2, 5) and (3, 4), their own row strides (D + 8, D + 24) and
    modulation tables; segment `none_seg` has shift = scale = None, the other has them set. Each output against the same fp64
    reference and bound as the single call (test_layernorm_modulate_per_element), sentinel guards on both outputs."""
    segs = []
    for i, (B, R, pad) in enumerate([(2, 5, 8), (3, 4, 24)]):
        x, table, shift, scale = ln_case(B, R, D, xdtype, seed=D + 17 * i + 1)
        _, xv = guarded3(x, 2, D + pad, NAN, xdtype, gpu)
        tab = table.to(gpu)
        mod = i != none_seg
        segs.append(dict(B=B, R=R, x=x, xv=xv, sh=tab[:, 4 : 4 + D] if mod else None, sc=tab[:, 4 + D : 4 + 2 * D] if mod else None,
                         shift=shift if mod else None, scale=scale if mod else None))

    def run():
        o = [torch.full((s["B"], s["R"] + 2, D + 16), SENT, dtype=BF16, device=gpu) for s in segs]
        a, b = segs
        ops.layernorm_modulate_pair(a["xv"], o[0][:, : a["R"], :D], a["sh"], a["sc"], b["xv"], o[1][:, : b["R"], :D], b["sh"], b["sc"])
        return o

    outs = twice(run)
    for i, (s, obuf) in enumerate(zip(segs, outs)):
        y, by = layernorm_ref(s["x"], s["shift"], s["scale"])
        check_bound(f"layernorm pair segment {i} ({'plain' if i == none_seg else 'modulated'}) D={D} {ids_dt(xdtype)}",
                    obuf[:, : s["R"], :D], y, ln_bound(y, by))
        assert outside3_is(obuf, s["R"], D, SENT), f"segment {i}: wrote outside the output view"


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16_out", "e4m3_out"])
def test_layernorm_refusals_launch_nothing(ops, gpu, fp8):
    """Rejected on the host, on real buffers, and the output keeps its sentinel: D = 12 and D = 8200 RT_E_SHAPE, D = 0 RT_E_BADARG,
    exactly one of shift / scale RT_E_BADARG, ldx % 8 != 0 RT_E_ALIGN; the bf16 and the e4m3 entry."""
    from reptext_amd import native

    B, R = 2, 3

    def attempt(D, ldx, shift=False, scale=False):
        x = torch.zeros(B, R, ldx, device=gpu, dtype=BF16)[:, :, :D]
        out = torch.full((B, R, max(D, 8) + 8), 0x31 if fp8 else SENT, device=gpu, dtype=torch.uint8 if fp8 else BF16)
        mod = torch.zeros(B, 2 * max(D, 8), device=gpu)
        sh = mod[:, :D] if shift else None
        sc = mod[:, max(D, 8) : max(D, 8) + D] if scale else None
        rs = torch.full((B * R,), SENT, device=gpu)
        with pytest.raises(native.NativeCallError) as e:
            if fp8:
                ops.layernorm_modulate_fp8(x, out.view(torch.float8_e4m3fn)[:, :, :D], rs, sh, sc)
            else:
                ops.layernorm_modulate(x, out[:, :, :D], sh, sc)
        torch.cuda.synchronize()
        assert same_bits(out, torch.full_like(out, 0x31 if fp8 else SENT)) and same_bits(rs, torch.full_like(rs, SENT))
        return e.value.code

    assert attempt(12, 16) == native.RT_E_SHAPE
    assert attempt(8200, 8200) == native.RT_E_SHAPE
    assert attempt(0, 8) == native.RT_E_BADARG
    assert attempt(64, 64, shift=True) == native.RT_E_BADARG
    assert attempt(64, 68) == native.RT_E_ALIGN


# ------------------------------------------------------------------------------------------------ q/k RMSNorm + RoPE
# The excess of |got - ref| over 2^-8 |ref| + QK_COUNTED 2^-23 (|a cos| + |b sin|), relative to |a cos| + |b sin|: what the device
# rsqrtf adds to the counted roundings of rt_qk_norm_rope8. Measured on an MI355X over every case of
# test_qk_rmsnorm_rope_per_element (each prints its own; run with -s), worst at the shape noted:
MEASURED_QK_RSQRT_EXCESS = 0.0      # MI355X: nothing above the counted terms in any case (largest (2, 37, 12, 3)); counted terms alone
QK_SHAPES = [(1, 1, 0, 1), (2, 5, 0, 1), (2, 37, 37, 3), (2, 37, 12, 3), (1, 33, 1, 5)]


def qk_buffer(B, S, H, single, seed):
    """bf16 [B, S + 2, ld] on the CPU: N(0, 1) in the q and k columns of rows < S (one q head all zero), and in every other place —
    v, the mlp columns, the pad columns, the rows behind S — recognisable finite values ((7 col + 13 row) % 251 - 125) / 8, which an
    in-place kernel must leave bit for bit."""
    d = H * 128
    q_off, k_off, ld = qk_layout(single, d)
    g = torch.Generator().manual_seed(seed)
    r, c = torch.arange(B * (S + 2))[:, None], torch.arange(ld)[None, :]
    buf = (((7 * c + 13 * r) % 251 - 125).float() / 8).reshape(B, S + 2, ld).to(BF16)
    buf[:, :S, q_off : q_off + d] = torch.randn(B, S, d, generator=g).to(BF16)
    buf[:, :S, k_off : k_off + d] = (torch.randn(B, S, d, generator=g) * 2).to(BF16)
    buf[0, 0, q_off : q_off + 128] = 0
    return buf


def qk_bound(ref, mag):
    return 2.0 ** -8 * ref.abs() + (QK_COUNTED * U23 + 4 * MEASURED_QK_RSQRT_EXCESS) * mag


@pytest.mark.parametrize("single", [False, True], ids=["double_block", "single_block"])
@pytest.mark.parametrize("B,S,T,H,pos0", [s + (0,) for s in QK_SHAPES] + [(2, 37, 12, 3, 4000)])
def test_qk_rmsnorm_rope_per_element(ops, gpu, B, S, T, H, pos0, single):
    """ops.qk_rmsnorm_rope, in place, both layouts (double block: q at 0, k at d, v behind; single block: k at 0, q at 2 d,
    ld = 7 d + 8), against support_kernels.qk_norm_rope_ref. Bound per element:
        2^-8 |ref| + (QK_COUNTED 2^-23 + 4 MEASURED_QK_RSQRT_EXCESS) (|a cos| + |b sin|)
    2^-8 |ref|: the bf16 rounding of the output. QK_COUNTED = 6: the roundings of rt_qk_norm_rope8 counted at support_kernels.
    QK_COUNTED. The last: the device rsqrtf, measured (see MEASURED_QK_RSQRT_EXCESS). Rows T - 1 and T, the last row, the all-zero
    head (zeros out, finite) are elements like any other; with the weight sets O(1) apart, the wrong set is an O(1) error there.
    Everything outside the q and k columns of rows < S is unchanged bit for bit."""
    d = H * 128
    q_off, k_off, ld = qk_layout(single, d)
    host = qk_buffer(B, S, H, single, seed=S + H)
    w = qk_weights(S)
    cos, sin = qk_tables(S, T, pos0)
    wd = [t.to(gpu) for t in w]
    cd, sd = cos.to(gpu), sin.to(gpu)

    def run():
        buf = host.clone().to(gpu)
        ops.qk_rmsnorm_rope(buf[:, :S], q_off, k_off, H, T, wd[0] if T > 0 else None, wd[1] if T > 0 else None, wd[2], wd[3], cd, sd,
                            eps=QK_EPS)
        return buf

    got = twice(run).cpu()
    what = f"qk_rmsnorm_rope {'single' if single else 'double'} B={B} S={S} T={T} H={H} pos0={pos0}"
    worst = 0.0
    for name, off, wt, wi in (("q", q_off, w[0], w[2]), ("k", k_off, w[1], w[3])):
        x = host[:, :S, off : off + d].reshape(B, S, H, 128)
        ref, mag = qk_norm_rope_ref(x, wt, wi, T, cos, sin, QK_EPS)
        out = got[:, :S, off : off + d].reshape(B, S, H, 128).double()
        excess = (((out - ref).abs() - 2.0 ** -8 * ref.abs()) / mag.clamp_min(1e-300) - QK_COUNTED * U23)[mag > 0]
        worst = max(worst, float(excess.max()) if excess.numel() else 0.0)
        check_bound(f"{what} {name}", out, ref, qk_bound(ref, mag))
    print(f"[rsqrt] {what}: excess over the counted terms {max(worst, 0.0):.3e} (MEASURED_QK_RSQRT_EXCESS {MEASURED_QK_RSQRT_EXCESS:.3e})")
    assert bool((got[0, 0, q_off : q_off + 128] == 0).all()), "the all-zero head"
    keep = torch.ones(host.shape, dtype=torch.bool)
    keep[:, :S, q_off : q_off + d] = False
    keep[:, :S, k_off : k_off + d] = False
    assert same_bits(got[keep], host[keep]), "changed something outside the q and k columns"


# ------------------------------------------------------------------------------------------------ GEMV
# Worst |silu_f(x) - silu(x)| / |silu(x)| of the kernel's fp32 SiLU (x / (1 + __expf(-x))) over x = 64 values across [-8, 8], through a
# K = 8 launch with one-hot weights (each output is one silu_f(x) and seven exact zeros), measured on an MI355X by
# test_gemv_silu_coefficient_measurement below (run it with -s; the figure is printed). The bound allows 4x that.
# Measured 3.412e-07 (MI355X, B = N = K = 8, x = linspace(-8, 8, 64)) -> SILU_SLACK 1.365e-06.
MEASURED_SILU_COEFF = 3.412e-07
SILU_SLACK = 4 * MEASURED_SILU_COEFF
GEMV_SHAPES = [(1, 1, 8), (3, 15, 520), (8, 17, 512), (9, 33, 3072), (2, 1000, 3072)]
GEMV_FORMS = ["plain", "silu_in", "silu_out_accumulate", "no_bias"]


def silu64(v):
    v = v.double()
    return v * torch.sigmoid(v)


def test_gemv_silu_coefficient_measurement(ops, gpu):
    """Measures MEASURED_SILU_COEFF (see there) and holds the kernel to 4x the recorded value."""
    x = torch.linspace(-8.0, 8.0, 64).reshape(8, 8)
    w = torch.eye(8).to(BF16)
    y = torch.empty(8, 8, device=gpu)
    ops.gemv(x.to(gpu), w.to(gpu), None, y, silu_in=True)
    ref = silu64(x)
    rel = ((y.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300)).max()
    print(f"[silu] worst |silu_f(x) - silu(x)| / |silu(x)| over [-8, 8]: {float(rel):.3e}  (MEASURED_SILU_COEFF {MEASURED_SILU_COEFF:.3e}, "
          f"SILU_SLACK {SILU_SLACK:.3e})")
    assert float(rel) <= SILU_SLACK


@pytest.mark.parametrize("form", GEMV_FORMS)
@pytest.mark.parametrize("B,N,K", GEMV_SHAPES)
def test_gemv_per_element(ops, gpu, B, N, K, form):
    """ops.gemv: out[b, n] (+)= post(sum_k pre(x[b, k]) w[n, k] + bias[n]) against fp64, per element. x, w and out are views with
    ldx = K + 8, ldw = K + 8, ldy = N + 5: NaN behind the rows of x and w and in an extra row, the sentinel around out. B = 9 takes
    the wrapper's second launch (at most 8 rows, and 16384 / K, per launch); N = 15, 17, 33 end inside a wave's four rows and inside a
    workgroup's sixteen. Bound:
        (K + 16) 2^-23 mag,   mag = sum_k |pre(x)| |w| + |bias| (+ |y_old| with accumulate)
    K + 16 fp32 roundings of at most 2^-23 each, relative to the sum of the absolute addends (support_kernels.gemm_epilogue_ref's
    mag). silu_in: the fp32 SiLU is relative to each term, + SILU_SLACK sum_k |silu(x)| |w|. silu_out: the pre-activation v carries
    the above through |silu'| <= 1.1, + SILU_SLACK |v| for the SiLU itself. |x| <= 5 and |v| <= 8: the range SILU_SLACK was
    measured on."""
    g = torch.Generator().manual_seed(B * 1000 + N + K)
    x = torch.randn(B, K, generator=g).clamp(-5.0, 5.0)
    w = (torch.randn(N, K, generator=g) * (0.02 if K > 8 else 0.5)).to(BF16)
    bias = None if form == "no_bias" else (torch.randn(N, generator=g) * 0.5).to(BF16)
    y_old = torch.randn(B, N, generator=g)
    silu_in, silu_out = form == "silu_in", form == "silu_out_accumulate"
    xd = guarded_rows(x, K + 8, 1, NAN, F32, gpu)
    wd = guarded_rows(w, K + 8, 1, NAN, BF16, gpu)
    bd = None if bias is None else bias.to(gpu)

    def run():
        obuf = torch.full((B + 1, N + 5), SENT, dtype=F32, device=gpu)
        if silu_out:
            obuf[:B, :N] = y_old.to(gpu)
        ops.gemv(xd[:B, :K], wd[:N, :K], bd, obuf[:B, :N], silu_in=silu_in, silu_out=silu_out, accumulate=silu_out)
        return obuf

    obuf = twice(run)
    pre = silu64(x) if silu_in else x.double()
    v = pre @ w.double().t()
    mag = pre.abs() @ w.double().abs().t()
    bound = torch.zeros_like(v)
    if silu_in:
        bound = bound + SILU_SLACK * mag
    if bias is not None:
        v, mag = v + bias.double(), mag + bias.double().abs()
    if silu_out:
        assert float(v.abs().max()) <= 8.0
        ref = y_old.double() + silu64(v)
        bound = 1.1 * (bound + (K + 16) * U23 * mag) + SILU_SLACK * v.abs() + (K + 16) * U23 * y_old.double().abs()
    else:
        ref = v
        bound = bound + (K + 16) * U23 * mag
    check_bound(f"gemv {form} B={B} N={N} K={K}", obuf[:B, :N], ref, bound)
    assert outside_is(obuf, B, N, SENT), "wrote outside the output view"
