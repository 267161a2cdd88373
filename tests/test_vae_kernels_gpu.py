"""The AutoencoderKL's MFMA kernels — rt_conv2d_nhwc on both of its kernels (conv_nhwc_kernel<4> / <2> of csrc/vae.hip and the convolution
form of rt_gemm_bf16, csrc/gemm_bf16.hip CONV on Geo256 / Geo128) and rt_vae_attention (csrc/vae_attention.hip) — against fp64 references,
judged PER ELEMENT, on guarded buffers: NaN wherever a kernel must not read (or must read zeros through its buffer descriptor), a
sentinel wherever it must not write.

Convolution. Reference (support_kernels.conv_ref): fp64 F.conv2d of the bf16 values the kernel reads, in the header's three geometries,
and `mag`, the same convolution of |x| with |w| plus |bias| plus |res|. Bound, per element, with K = ks * ks * Cin:
    fp32 output   |got - ref| <= (K + 16) * 2^-23 * mag
    bf16 output   the same + 2^-8 |ref|
K * 2^-23 * mag is the classical bound of K fp32 additions in any order with unit roundoff 2^-23 (it covers an MFMA that truncates), the
16 covers the epilogue's two fp32 additions with room to spare, 2^-8 |ref| >= half a bf16 ulp of ref is the output rounding. Nothing
in it is measured. Weights are independent random values per tap, input and output channel and x is N(0,1) without any symmetry, so a
swapped dy / dx, a shifted tap or a transposed weight index cannot cancel.
Buffers: x is a zero-haloed image inside a flat NaN-filled allocation with at least (W + 4) * Cin NaN elements in front of and behind
it — the rows the GEMM form's shifted loads reach outside the image, which its buffer descriptor must turn into zeros; w, bias and res
(NaN halo) are NaN-padded in the same way; y is a sentinel-haloed image inside a sentinel-filled allocation: "halo pixels are computed
and NOT stored".

Attention. Reference: support_kernels.attention_ref with H = 1, Dh = C. Bound, per element, as tests/test_attention_edges_gpu.py has it:
    |got - ref| <= 2^-8 |ref| + 2^-8 sum_j p_j |v_j| + slack
p the fp64 softmax row. First term: the bf16 rounding of the output. Second: P reaches the second MFMA as bf16 (vae_attention.hip:
`pf[s2][j] = (__bf16)p`, the B operand of the V^T P^T product) — every p_j is rounded by at most 2^-9 relative, whatever power of two
the deferred rescale has left it scaled by, which moves the numerator by at most 2^-9 sum_j p_j |v_j|; the normaliser is the fp32 sum
of the UNROUNDED p, so the other 2^-9 is headroom for the 1 / l multiply and the rounding of v p products the MFMA accumulates.
slack: the fp32 exp2, the LDS exchange's partial-score sum and the accumulation; see MEASURED_EXCESS."""
import math

import pytest
import torch

from support_kernels import BF16, F32, NAN, SENT, attention_ref, check_bound, conv_ref, halo_is, haloed, same_bits, twice

pytestmark = pytest.mark.gpu


class conv_variant:
    """rt_conv2d_variant(mode) for the duration of a with-block; the previous mode is restored whatever happens."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from reptext_amd import native

        self.lib = native.load()
        self.prev = self.lib.rt_conv2d_variant(-1)
        self.lib.rt_conv2d_variant(self.mode)

    def __exit__(self, *exc):
        self.lib.rt_conv2d_variant(self.prev)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ================================================================================================ convolution
def up8(n):
    return (n + 7) // 8 * 8


def guarded_flat(vals, fill, pad, device):
    """`vals` as a view of a flat allocation filled with `fill`, `pad` elements (a multiple of 8: the view stays 16-byte aligned) in front
    of and behind it. Returns (allocation, view)."""
    assert pad % 8 == 0
    flat = torch.full((2 * pad + vals.numel(),), fill, dtype=vals.dtype)
    flat[pad : pad + vals.numel()] = vals.reshape(-1)
    flat = flat.to(device)
    view = flat[pad : pad + vals.numel()].view(vals.shape)
    assert view.data_ptr() % 16 == 0
    return flat, view


class Conv:
    """One convolution problem: its true values on the CPU (exactly what the kernel reads), the fp64 reference, the guarded device buffers."""

    def __init__(self, B, Hs, Ws, Cin, Cout, ks, stride, up, out_f32, bias, res, seed, device):
        self.B, self.Hs, self.Ws, self.Cin, self.Cout, self.ks, self.stride, self.up, self.out_f32 = B, Hs, Ws, Cin, Cout, ks, stride, up, out_f32
        self.Ho, self.Wo = (Hs // 2, Ws // 2) if stride == 2 else (2 * Hs, 2 * Ws) if up else (Hs, Ws)
        self.K, self.dev = ks * ks * Cin, device
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)
        self.x = rn(B, Hs, Ws, Cin).to(BF16)
        self.w = (rn(Cout, ks, ks, Cin) / self.K ** 0.5).to(BF16)
        self.bias = rn(Cout).to(BF16) if bias else None
        self.res = rn(B, self.Ho, self.Wo, Cout).to(BF16) if res else None
        self.ref, self.mag = conv_ref(self.x, self.w, self.bias, self.res, stride, up)
        self.bound = (self.K + 16) * 2.0 ** -23 * self.mag + (0.0 if out_f32 else 2.0 ** -8) * self.ref.abs()
        # ---- device side. The rows a shifted load of the GEMM form reaches in front of / behind the image are NaN, inside the allocation
        self.inputs = []
        self.d_x = self._input(haloed(self.x, 0.0), up8((Ws + 4) * Cin))
        self.d_w = self._input(self.w, 64)
        self.d_bias = self._input(self.bias, 8) if bias else None
        self.d_res = self._input(haloed(self.res, NAN), up8((self.Wo + 4) * Cout)) if res else None
        self.ypad = up8((self.Wo + 4) * Cout)

    def _input(self, vals, pad):
        flat, view = guarded_flat(vals, NAN, pad, self.dev)
        self.inputs.append((flat, flat.clone()))
        return view

    def new_y(self, init=None):
        """A sentinel-filled allocation and its haloed [B, Ho+2, Wo+2, Cout] view (sentinel halo; `init`: what the interior holds first)."""
        dt = F32 if self.out_f32 else BF16
        return guarded_flat(haloed(init if init is not None else (self.B, self.Ho, self.Wo, self.Cout), SENT, dtype=dt), SENT, self.ypad, self.dev)

    def launch(self, in_place=False):
        """One call on fresh output buffers. in_place: res = y, as the ResnetBlock calls it. Returns (allocation, haloed view)."""
        from reptext_amd import native

        flat, y = self.new_y(self.res if in_place else None)
        res = y if in_place else self.d_res
        native.call("rt_conv2d_nhwc", self.d_x.data_ptr(), self.d_w.data_ptr(), self.d_bias.data_ptr() if self.d_bias is not None else None,
                    res.data_ptr() if res is not None else None, y.data_ptr(), self.B, self.Hs, self.Ws, self.Cin, self.Cout, self.ks,
                    self.stride, self.up, self.out_f32, stream())
        torch.cuda.synchronize()
        return flat, y

    def check(self, what, in_place=False):
        """Twice with equal bits; the interior inside the bound; halo and guards still the sentinel; every input keeps its bits.
        Returns the interior."""
        flat, y = twice(lambda: self.launch(in_place))
        check_bound(what, y[:, 1:-1, 1:-1], self.ref, self.bound)
        assert halo_is(y, SENT), f"{what}: a halo pixel of y was stored"
        assert same_bits(flat[: self.ypad], torch.full_like(flat[: self.ypad], SENT)), f"{what}: wrote in front of y"
        assert same_bits(flat[-self.ypad :], torch.full_like(flat[-self.ypad :], SENT)), f"{what}: wrote behind y"
        for buf, before in self.inputs:
            assert same_bits(buf, before), f"{what}: the kernel wrote to an input"
        return y[:, 1:-1, 1:-1].clone()


def run_conv_case(gpu, what, seed, B, Hs, Ws, Cin, Cout, ks=3, stride=1, up=0, out_f32=0, bias=True, res=True):
    """Every assertion of a case. A stride-1, non-upsampling, bf16-output case with Cout >= 64 is served by either kernel: it runs on the
    GEMM's convolution form (variant 1) and on conv_nhwc_kernel (variant 0), both judged against fp64, with equal bits. Everything else
    has one kernel, whatever the variant. With a residual and bf16 output it also runs in place, with the bits of the out-of-place run."""
    c = Conv(B, Hs, Ws, Cin, Cout, ks, stride, up, out_f32, bias, res, seed, gpu)
    both = stride == 1 and not up and not out_f32 and Cout >= 64
    outs = {}
    for mode in (1, 0) if both else (1,):
        name = f"{what} [{('gemm form' if mode else 'direct kernel') if both else 'direct kernel'}]"
        with conv_variant(mode):
            outs[mode] = c.check(name)
            if res and not out_f32:
                assert same_bits(c.check(name + " in place", in_place=True), outs[mode]), f"{name}: in place over res differs"
    if both:
        assert same_bits(outs[0], outs[1]), f"{what}: the two kernels differ"


# Stride 1 at B = 2, H = 9, W = 15. conv_nhwc_kernel: 270 output rows — tile 0 holds all of image 0 and 121 rows of image 1, tile 1 is 14
# ragged rows. GEMM form: 2 * 11 * 17 = 374 haloed rows — a ragged second tile whose edge falls in the middle of image 1's rows.
# Cin = 192 is three K-tiles per tap (both LDS buffers; cv_c0 wraps into the next tap and into the next image row), Cin = 64 one.
# id: kernel paths (direct kernel / GEMM form), then the shape.                  Cin Cout ks bias  res
STRIDE1 = {
    "direct2+Geo128/k3_cin64_cout64":                                             (64, 64, 3, True, True),
    "direct2+Geo128/k3_cin192_cout128_last_narrow_width":                         (192, 128, 3, True, True),
    "direct4+Geo256/k3_cin192_cout132_one_live_group_in_third_wave_column":       (192, 132, 3, True, True),
    "direct4+Geo256/k3_cin192_cout260_second_tile_column_narrow_store":           (192, 260, 3, True, True),
    "direct4+Geo256/k3_cin64_cout260_no_bias_no_res":                             (64, 260, 3, False, False),
    "direct2+Geo128/k1_cin64_cout64_no_bias":                                     (64, 64, 1, False, True),
    "direct2+Geo128/k1_cin192_cout128_no_res":                                    (192, 128, 1, True, False),
    "direct4+Geo256/k1_cin64_cout132":                                            (64, 132, 1, True, True),
    "direct4+Geo256/k1_cin192_cout260_second_tile_column":                        (192, 260, 1, True, True),
}


@pytest.mark.parametrize("name", list(STRIDE1))
def test_conv_stride1_both_kernels(gpu, name):
    Cin, Cout, ks, bias, res = STRIDE1[name]
    run_conv_case(gpu, "stride1 " + name, 100 + list(STRIDE1).index(name), 2, 9, 15, Cin, Cout, ks=ks, bias=bias, res=res)


# What only conv_nhwc_kernel serves: fp32 output (Cout = 4, ks = 3 is the decoder's conv_out: <2> with one live column group),
# Cout < 64, the fused nearest-2x upsample (2 x 5 x 7 -> 10 x 14: odd source sizes) and stride 2 (2 x 18 x 30 -> 9 x 15).
#                                                                   Hs  Ws  Cin Cout ks stride up f32 bias  res
DIRECT_ONLY = {
    "out_f32/direct2/k3_cin192_cout4_conv_out":                      (9, 15, 192, 4, 3, 1, 0, 1, True, False),
    "out_f32/direct2/k3_cin64_cout4_no_bias":                        (9, 15, 64, 4, 3, 1, 0, 1, False, False),
    "out_f32/direct2/k3_cin192_cout128_res":                         (9, 15, 192, 128, 3, 1, 0, 1, True, True),
    "out_f32/direct4/k3_cin192_cout132_res":                         (9, 15, 192, 132, 3, 1, 0, 1, True, True),
    "out_f32/direct4/k1_cin64_cout260":                              (9, 15, 64, 260, 1, 1, 0, 1, True, False),
    "narrow_cout/direct2/k3_cin64_cout32_bf16":                      (9, 15, 64, 32, 3, 1, 0, 0, True, True),
    "narrow_cout/direct2/k3_cin192_cout4_bf16":                      (9, 15, 192, 4, 3, 1, 0, 0, True, True),
    "upsample/direct2/k3_cin192_cout128":                            (5, 7, 192, 128, 3, 1, 1, 0, True, False),
    "upsample/direct4/k3_cin192_cout260_res":                        (5, 7, 192, 260, 3, 1, 1, 0, True, True),
    "upsample/direct2/k3_cin64_cout64_no_bias":                      (5, 7, 64, 64, 3, 1, 1, 0, False, True),
    "upsample/direct4/k3_cin64_cout132_f32":                         (5, 7, 64, 132, 3, 1, 1, 1, True, False),
    "stride2/direct2/k3_cin192_cout128":                             (18, 30, 192, 128, 3, 2, 0, 0, True, False),
    "stride2/direct4/k3_cin192_cout132_res":                         (18, 30, 192, 132, 3, 2, 0, 0, True, True),
    "stride2/direct4/k3_cin64_cout260_no_bias":                      (18, 30, 64, 260, 3, 2, 0, 0, False, False),
    "stride2/direct2/k3_cin64_cout64_f32":                           (18, 30, 64, 64, 3, 2, 0, 1, True, True),
}


@pytest.mark.parametrize("name", list(DIRECT_ONLY))
def test_conv_direct_kernel_only(gpu, name):
    Hs, Ws, Cin, Cout, ks, stride, up, f32, bias, res = DIRECT_ONLY[name]
    run_conv_case(gpu, name, 200 + list(DIRECT_ONLY).index(name), 2, Hs, Ws, Cin, Cout, ks=ks, stride=stride, up=up, out_f32=f32, bias=bias, res=res)


# Images so small that (nearly) every tap of a pixel is halo. H = W = 1: every tap but the centre reads halo, and conv_w2 = 3 is the
# GEMM form's minimum (18 haloed rows, 2 of them stored). B = 2 throughout.
#                                                                   Hs Ws Cin Cout ks stride up f32 bias  res
DEGENERATE = {
    "degenerate/direct4+Geo256/1x1_k3_cin192_cout132":               (1, 1, 192, 132, 3, 1, 0, 0, True, True),
    "degenerate/direct2+Geo128/1x1_k3_cin64_cout128":                (1, 1, 64, 128, 3, 1, 0, 0, True, False),
    "degenerate/direct2+Geo128/1x1_k1_cin64_cout64":                 (1, 1, 64, 64, 1, 1, 0, 0, True, True),
    "degenerate/direct4+Geo256/1x1_k1_cin192_cout260":               (1, 1, 192, 260, 1, 1, 0, 0, False, True),
    "degenerate/direct2+Geo128/1x5_k3_cin192_cout128":               (1, 5, 192, 128, 3, 1, 0, 0, True, True),
    "degenerate/direct4+Geo256/1x5_k3_cin64_cout260":                (1, 5, 64, 260, 3, 1, 0, 0, True, True),
    "degenerate/direct2/1x1_k3_cin192_cout4_f32_conv_out":           (1, 1, 192, 4, 3, 1, 0, 1, True, False),
    "degenerate/direct2/stride2_from_2x2_cin192_cout64":             (2, 2, 192, 64, 3, 2, 0, 0, True, True),
    "degenerate/direct4/stride2_from_2x2_cin64_cout132":             (2, 2, 64, 132, 3, 2, 0, 0, True, False),
    "degenerate/direct4/upsample_from_1x1_cin64_cout132":            (1, 1, 64, 132, 3, 1, 1, 0, True, True),
    "degenerate/direct2/upsample_from_1x1_cin192_cout128":           (1, 1, 192, 128, 3, 1, 1, 0, True, False),
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_conv_degenerate_sizes(gpu, name):
    Hs, Ws, Cin, Cout, ks, stride, up, f32, bias, res = DEGENERATE[name]
    run_conv_case(gpu, name, 300 + list(DEGENERATE).index(name), 2, Hs, Ws, Cin, Cout, ks=ks, stride=stride, up=up, out_f32=f32, bias=bias, res=res)


def test_conv_variant_is_restored(gpu):
    """conv_variant puts the previous mode back also when the block raises."""
    from reptext_amd import native

    lib = native.load()
    before = lib.rt_conv2d_variant(-1)
    with pytest.raises(RuntimeError):
        with conv_variant(1 - before):
            assert lib.rt_conv2d_variant(-1) == 1 - before
            raise RuntimeError("inside the block")
    assert lib.rt_conv2d_variant(-1) == before


# ================================================================================================ rt_vae_attention
# Worst excess of |got - ref| over the first two terms of the bound, across every case below (C x HW sweep, late and early dominant
# keys), measured on an MI355X (run this file with -s: every case prints its own excess): 0.0 in all 24 cases (worst err/bound 0.82,
# early dominant key, C = 128, HW = 64). With nothing measured to multiply by 4, the slack is 2^-20 max|v| of the case's data (about 4.5e-6 here), the rule
# of test_attention_edges_gpu.attn_slack.
MEASURED_EXCESS = 0.0


def attn_slack(vmax):
    return 4 * MEASURED_EXCESS if MEASURED_EXCESS > 0 else 2.0 ** -20 * vmax


AB = 2
CS = [128, 256, 512]
HWS = [32, 64, 96, 160]          # one tile (prologue and drain, no loop); both ring slots once each; a slot reused; five tiles


def make_qkv(C, HW, seed, dominant=()):
    """bf16 [AB, HW, 3C] on the CPU, q scaled by 2 (a sharper softmax than N(0,1) scores). dominant = (b, query row, key): that key becomes
    the query row's direction, so its score is 4 sqrt(C) >= 45 above the rest."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(AB, HW, 3 * C, generator=g)
    qkv[..., :C] *= 2.0
    qkv = qkv.to(BF16)
    for b, row, key in dominant:
        qkv[b, key, C : 2 * C] = qkv[b, row, :C]
    return qkv


def attn_reference(qkv, C):
    Bn, HW, _ = qkv.shape
    q, k, v = (qkv[..., i * C : (i + 1) * C].float().reshape(Bn, HW, 1, C) for i in range(3))
    ref, pv = attention_ref(q, k, v)
    return ref, pv, float(v.abs().max())


def fused_buffer(qkv, device):
    """[Bn, HW + 40, 3C + 64] with NaN in the 40 rows (more than one 32-key tile) behind HW of every batch entry and in the pad columns:
    ld = 3C + 64, a padded batch stride. Returns (buffer, q, k, v views)."""
    Bn, HW, C3 = qkv.shape
    buf = torch.full((Bn, HW + 40, C3 + 64), NAN, dtype=BF16)
    buf[:, :HW, :C3] = qkv
    buf = buf.to(device)
    C = C3 // 3
    return (buf,) + tuple(buf[:, :HW, i * C : (i + 1) * C] for i in range(3))


def attn_launch(q, k, v, C, device):
    """One call into a fresh [Bn, HW + 3, C + 8] sentinel-filled output; returns that buffer."""
    from reptext_amd import native

    Bn, HW, _ = q.shape
    obuf = torch.full((Bn, HW + 3, C + 8), SENT, dtype=BF16, device=device)
    native.call("rt_vae_attention", q.data_ptr(), k.data_ptr(), v.data_ptr(), obuf.data_ptr(), q.stride(1), q.stride(0), obuf.stride(1),
                obuf.stride(0), Bn, HW, C, 1.0 / math.sqrt(C), stream())
    torch.cuda.synchronize()
    return obuf


def run_attention(what, qkv, C, device):
    """Guarded buffers, twice; bound (the excess over its first two terms printed first), guards, inputs untouched; every batch entry has
    the bits of its own B = 1 launch. Returns the output on the CPU."""
    Bn, HW, _ = qkv.shape
    buf, q, k, v = fused_buffer(qkv, device)
    before = buf.clone()
    obuf = twice(lambda: attn_launch(q, k, v, C, device))
    got = obuf[:, :HW, :C].double().cpu()
    ref, pv, vmax = attn_reference(qkv, C)
    base = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * pv
    slack = attn_slack(vmax)
    excess = float(((got - ref).abs() - base).max())
    print(f"[vae attention] {what}: excess over 2^-8|ref| + 2^-8 sum p|v| {max(excess, 0.0):.3e} (slack {slack:.3e})")
    check_bound(what, got, ref, base + slack)
    m = torch.ones(obuf.shape, dtype=torch.bool, device=device)
    m[:, :HW, :C] = False
    assert same_bits(obuf[m], torch.full_like(obuf[m], SENT)), f"{what}: wrote outside [:HW, :C] of the output"
    assert same_bits(buf, before), f"{what}: the kernel wrote to its inputs"
    for b in range(Bn):
        _, q1, k1, v1 = fused_buffer(qkv[b : b + 1], device)
        assert same_bits(attn_launch(q1, k1, v1, C, device)[0], obuf[b]), f"{what}: entry {b} differs from its B = 1 launch"
    return got


@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_vae_attention_tiles(gpu, C, HW):
    run_attention(f"vae attention C={C} HW={HW}", make_qkv(C, HW, 5000 + C + HW), C, gpu)


def dominant_rows(HW, key):
    """One query row per batch entry, in different workgroups where there is more than one."""
    return [(0, 5, key), (1, HW - 2, key)]


@pytest.mark.parametrize("HW", [64, 160])
@pytest.mark.parametrize("C", CS)
def test_vae_attention_late_dominant_key(gpu, C, HW):
    """The LAST key is aligned with one query row: that row's maximum jumps by far more than RESCALE_THR on the last tile, after
    HW / 32 - 1 tiles of accumulation, so the deferred rescale fires there."""
    rows = dominant_rows(HW, HW - 1)
    qkv = make_qkv(C, HW, 6000 + C + HW, dominant=rows)
    got = run_attention(f"vae attention late key C={C} HW={HW}", qkv, C, gpu)
    for b, row, key in rows:                                       # the row is (almost exactly) the value row of the dominant key
        assert float((got[b, row] - qkv[b, key, 2 * C :].double()).abs().max()) < 0.05, (b, row)


@pytest.mark.parametrize("HW", [64, 160])
@pytest.mark.parametrize("C", CS)
def test_vae_attention_early_dominant_key(gpu, C, HW):
    """Key 0 dominates one query row: its maximum is set on the first tile and never moves again, every later tile only adds
    exp2(score - max) ~ 0 terms."""
    rows = dominant_rows(HW, 0)
    qkv = make_qkv(C, HW, 7000 + C + HW, dominant=rows)
    got = run_attention(f"vae attention early key C={C} HW={HW}", qkv, C, gpu)
    for b, row, key in rows:
        assert float((got[b, row] - qkv[b, key, 2 * C :].double()).abs().max()) < 0.05, (b, row)
