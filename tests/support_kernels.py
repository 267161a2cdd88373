"""What the tests of tests/test_support_kernels_gpu.py, test_gemm_epilogue_gpu.py, test_attention_edges_gpu.py,
test_small_head_attention_edges_gpu.py and test_vae_kernels_gpu.py share: the fp64 references of the GEMM epilogue, of the convolution
and of attention, the per-element bound check, guarded buffers (NaN where a kernel must not read, a sentinel where it must not write), the bf16 error bound, ulp distances and the run-twice check. Further down, for test_token_passes_gpu.py and
test_e4m3_producers_gpu.py: batched guarded views, the fp64 references and fp32-evaluation bounds of LayerNorm + modulation and of q/k
RMSNorm + RoPE, the e4m3 grid (ulp_e4m3, finite bytes), the row-quantisation rule and the documented key order of the e4m3 V^T.
Next to attention_ref, for test_ip_attention_edges_gpu.py: the fp64 reference of the IP-Adapter term (ip_attention_ref64) with the
bf16 rounding of the normalised query done in fp64 (bf16_round64).
A plain helper module, not a test file."""
import torch

NAN = float("nan")
SENT = -7.0                      # exactly representable in bf16 and fp32; no kernel under test produces it from the inputs used
SENT_U8 = 249
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64, torch.uint8: torch.uint8,
        torch.int32: torch.int32}


def bits(t):
    """The tensor's storage as integers, so that NaN == NaN and -0.0 != 0.0."""
    return t.contiguous().view(_INT[t.dtype])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def twice(run):
    """run() launches the kernel from freshly restored buffers and returns its output tensor(s); the second launch must reproduce the
    first bit for bit. Returns the first result."""
    first = run()
    second = run()
    a = first if isinstance(first, (tuple, list)) else (first,)
    b = second if isinstance(second, (tuple, list)) else (second,)
    for u, v in zip(a, b):
        if u is not None:
            assert same_bits(u, v), "not bitwise repeatable"
    return first


def rel_l2(got, ref):
    got, ref = got.double().flatten(), ref.double().flatten()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def check_bf16(what, got, ref, slack, l2=True):
    """BF16(ref, slack): |got - ref| <= 2^-8 |ref| + slack elementwise (2^-8 |ref| >= half a bf16 ulp of ref, the slack is the kernel's
    fp32 evaluation), every output finite, and rel-L2 < 3e-3 (one bf16 output rounding). Prints the figures before it asserts."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + slack
    # the part of the error the slack has to carry: what is left after the output rounding's own share
    over = float((err - ref.abs() * 2.0 ** -8).max())
    r = rel_l2(got, ref)
    print(f"[support] {what}: max|err| {float(err.max()):.3e}  max err/bound {float((err / bound).max()):.3f}  "
          f"err beyond 2^-8|ref| {max(over, 0.0):.3e} (slack {slack:.1e})  rel-L2 {r:.3e}")
    assert finite, f"{what}: non-finite output"
    assert bool((err <= bound).all()), f"{what}: outside BF16(ref, {slack:g}), worst err/bound {float((err / bound).max()):.3f}"
    if l2:
        assert r < 3e-3, f"{what}: rel-L2 {r:.3e}"


def _ordered(t):
    """bf16 / fp32 bit patterns mapped to integers that are monotonic in the value (so a difference is a distance in ulps)."""
    i = bits(t).to(torch.int64)
    top = 1 << (15 if t.dtype == BF16 else 31)
    return torch.where(i < 0, -(i + top), i)


def ulp_distance(a, b):
    """Largest distance, in units in the last place of their common dtype, between two finite bf16 or fp32 tensors."""
    assert a.dtype == b.dtype and a.shape == b.shape
    assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all())
    return int((_ordered(a) - _ordered(b)).abs().max())


def f32_ulps_from(got, ref64, unit=None):
    """Largest |got - ref| in fp32 ulps of ref, ref in fp64 (the ulp of the binade ref lies in; fp32 normal range assumed). With `unit`
    the ulp is that of the magnitudes given there instead (for a sum that may cancel: its larger operand)."""
    ref64 = ref64.double()
    ulp = torch.exp2(torch.floor(torch.log2((ref64 if unit is None else unit.double()).abs().clamp_min(2.0 ** -126))) - 23)
    return float(((got.double() - ref64).abs() / ulp).max())


def guarded_rows(vals, ld, extra_rows, fill, dtype, device):
    """[rows + extra_rows, ld] filled with `fill`, `vals` ([rows, cols], or None) in its top-left corner."""
    rows, cols = vals.shape
    buf = torch.full((rows + extra_rows, ld), fill, dtype=dtype)
    buf[:rows, :cols] = vals.to(dtype)
    return buf.to(device)


def outside_is(buf, rows, cols, fill):
    """True when everything of the 2-D buffer outside [:rows, :cols] still holds `fill` exactly."""
    m = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    m[:rows, :cols] = False
    rest = buf[m]
    return same_bits(rest, torch.full_like(rest, fill))


def haloed(interior, fill, Cp=None, dtype=BF16, device="cpu"):
    """[B, H+2, W+2, Cp] holding `fill` in the one-pixel halo and in channels >= C, `interior` ([B, H, W, C], or its shape) inside."""
    shape = tuple(interior.shape) if isinstance(interior, torch.Tensor) else tuple(interior)
    B, H, W, C = shape
    buf = torch.full((B, H + 2, W + 2, Cp or C), fill, dtype=dtype, device=device)
    if isinstance(interior, torch.Tensor):
        buf[:, 1:-1, 1:-1, :C] = interior.to(device=device, dtype=dtype)
    return buf


def halo_is(buf, fill, C=None):
    """True when the halo pixels (all channels) and, with C given, the channels >= C of the interior hold `fill` exactly."""
    m = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    m[:, 1:-1, 1:-1, :(C if C is not None else buf.shape[3])] = False
    rest = buf[m]
    return same_bits(rest, torch.full_like(rest, fill))


def gn_pix_per_block(HW):
    """csrc/vae.hip gn_pix_per_block: pixels per workgroup of the GroupNorm statistics pass."""
    ppb = 32
    while (HW + ppb - 1) // ppb > 1024:
        ppb *= 2
    return ppb


def groupnorm_ref(x, gamma, beta, G, eps):
    """fp64 GroupNorm of x [B, H, W, C] (any device): returns (normalised * gamma + beta, the same through SiLU)."""
    B, H, W, C = x.shape
    xd = x.double().reshape(B, H * W, G, C // G)
    mean = xd.mean(dim=(1, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    n = ((xd - mean) / torch.sqrt(var + eps)).reshape(B, H, W, C) * gamma.double() + beta.double()
    return n, n * torch.sigmoid(n)


def check_bound(what, got, ref, bound):
    """|got - ref| <= bound elementwise (bound a tensor of ref's shape) and every output finite. Prints the worst err/bound before it
    asserts and returns it."""
    got, ref, bound = got.double().cpu(), ref.double().cpu(), bound.double().cpu()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))
    worst = float(ratio.max())
    at = tuple(int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
    print(f"[bound] {what}: max|err| {float(err[torch.isfinite(err)].max()) if finite else NAN:.3e}  worst err/bound {worst:.3f} at {at}")
    assert finite, f"{what}: non-finite output"
    assert worst <= 1.0, f"{what}: worst err/bound {worst:.3f} at {at} (got {float(got[at]):.6g}, ref {float(ref[at]):.6g}, bound {float(bound[at]):.3g})"
    return worst


def gelu_tanh_ref(v):
    """fp64 GELU, tanh form: 0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3)))."""
    v = v.double()
    return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))


def gemm_epilogue_ref(a, w, *, bias=None, gelu_from=None, gate=None, alpha=1.0, rowscale=None, res=None, add2=None, rows_per_batch=0,
                      a_scale=None, w_scale=None):
    """fp64 rt_gemm_group of CPU tensors holding exactly the values the kernel reads (any dtype; widened here), in the header's order:
    acc (* a_scale * w_scale) + bias -> GELU-tanh for n >= gelu_from -> gate -> alpha -> rowscale -> + res -> + add2.
      a [B, M, K], w [N, K], bias [N], gate [B * (M / rows), N] (rows = rows_per_batch or M), rowscale [rows] or [B, rows],
      res / add2 [B, M, N], a_scale [B * M], w_scale [N].
    Returns (ref, mag), both fp64 [B, M, N]. mag is the sum of the absolute values of every addend of the element: sum_k |a||w|
    carried through the same scalings (|a_scale w_scale|, |gate|, |alpha|, |rowscale|; GELU passes it on unchanged), plus |bias|
    (scaled like the product it is added to), |res| and |add2| — what a rounding error of the evaluation is relative to."""
    a, w = a.double(), w.double()
    B, M, K = a.shape
    N = w.shape[0]
    v = torch.einsum("bmk,nk->bmn", a, w)
    mag = torch.einsum("bmk,nk->bmn", a.abs(), w.abs())
    if a_scale is not None:
        s = a_scale.double().reshape(B, M, 1)
        v, mag = v * s, mag * s.abs()
    if w_scale is not None:
        s = w_scale.double().reshape(1, 1, N)
        v, mag = v * s, mag * s.abs()
    if bias is not None:
        v, mag = v + bias.double().reshape(1, 1, N), mag + bias.double().abs().reshape(1, 1, N)
    gf = N if gelu_from is None else max(int(gelu_from), 0)
    if gf < N:
        v = torch.cat([v[..., :gf], gelu_tanh_ref(v[..., gf:])], dim=-1)
    rows = rows_per_batch if rows_per_batch > 0 else M
    if gate is not None:
        s = gate.double().reshape(B, M // rows, 1, N).expand(B, M // rows, rows, N).reshape(B, M, N)
        v, mag = v * s, mag * s.abs()
    v, mag = v * float(alpha), mag * abs(float(alpha))
    if rowscale is not None:
        r = rowscale.double()
        r = r.reshape(1, rows).expand(B, rows) if r.dim() == 1 else r
        s = r.reshape(B, 1, rows).expand(B, M // rows, rows).reshape(B, M, 1)
        v, mag = v * s, mag * s.abs()
    if res is not None:
        v, mag = v + res.double(), mag + res.double().abs()
    if add2 is not None:
        v, mag = v + add2.double(), mag + add2.double().abs()
    return v, mag


def conv_ref(x, w, bias, res, stride, up):
    """fp64 rt_conv2d_nhwc of CPU tensors holding exactly the values the kernel reads (any dtype; widened here), in the kernel's own
    layouts without the halo: x [B, Hs, Ws, Cin], w [Cout, ks, ks, Cin], bias [Cout] or None, res [B, Ho, Wo, Cout] or None. The three
    geometries of include/reptext_hip.h: stride 1 pads ks // 2; up puts a nearest-2x upsample in front; stride 2 pads (0, 1, 0, 1).
    Returns (ref, mag), both fp64 [B, Ho, Wo, Cout]. mag is the same convolution of |x| with |w|, plus |bias|, plus |res|: the sum of
    the absolute values of every addend of the element — what a rounding error of the evaluation is relative to."""
    import torch.nn.functional as F

    ks = w.shape[1]

    def conv(xx, ww):
        xx, ww = xx.double().permute(0, 3, 1, 2), ww.double().permute(0, 3, 1, 2)
        if stride == 2:
            out = F.conv2d(F.pad(xx, (0, 1, 0, 1)), ww, stride=2)
        elif up:
            out = F.conv2d(F.interpolate(xx, scale_factor=2.0, mode="nearest"), ww, padding=ks // 2)
        else:
            out = F.conv2d(xx, ww, padding=ks // 2)
        return out.permute(0, 2, 3, 1).contiguous()

    ref, mag = conv(x, w), conv(x.abs(), w.abs())
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    return ref, mag


def attention_ref(q, k, v, scale=None):
    """fp64 softmax(q k^T scale) v of CPU tensors holding exactly the values the kernel reads: q [B or 1, Sq, H, Dh] (a leading 1 is
    one set of queries shared by the batch), k and v [B, Sk, H, Dh]. Returns (ref, pv) as [B, Sq, H * Dh]: the value and
    sum_j p_j |v_j| with p the fp64 softmax row — what the bf16 rounding of P (the second product's operand) and of the normaliser
    is relative to."""
    q, k, v = q.double(), k.double(), v.double()
    Bq, Sq, H, Dh = q.shape
    B, Sk = k.shape[:2]
    assert Bq in (1, B) and k.shape == v.shape == (B, Sk, H, Dh), (q.shape, k.shape, v.shape)
    sc = Dh ** -0.5 if scale is None else float(scale)
    ref, pv = torch.empty(B, Sq, H, Dh, dtype=F64), torch.empty(B, Sq, H, Dh, dtype=F64)
    for b in range(B):
        for h in range(H):                     # one [Sq, Sk] matrix at a time
            p = torch.softmax(q[b if Bq == B else 0, :, h] @ k[b, :, h].t() * sc, dim=-1)
            ref[b, :, h], pv[b, :, h] = p @ v[b, :, h], p @ v[b, :, h].abs()
    return ref.reshape(B, Sq, H * Dh), pv.reshape(B, Sq, H * Dh)


def bf16_round64(x):
    """The bf16 value nearest to each element of the fp64 tensor x (ties to even; the normal range is assumed), as fp64, and the
    distance of x to the nearest point halfway between two bf16 values, relative to |x| (inf where x is 0)."""
    m, e = torch.frexp(x.double())                 # x = m 2^e, |m| in [0.5, 1): m 2^8 has its 8 significant bits in front of the point
    y = m * 256.0
    margin = ((y - torch.floor(y)) - 0.5).abs() / y.abs()
    margin = torch.where(y == 0, torch.full_like(y, float("inf")), margin)
    return torch.ldexp(torch.round(y), e - 8), margin


def ip_qhat64(q, wq, eps):
    """fp64 q rsqrt(mean_128(q^2) + eps) wq of q [B, N, H, 128], before any rounding."""
    qd = q.double()
    return qd * torch.rsqrt((qd * qd).mean(-1, keepdim=True) + eps) * wq.double()


def ip_attention_ref64(q, wq, k, v, c, sm_scale, eps):
    """fp64 rt_ip_attention / _gated / _rows of CPU tensors holding exactly the values the kernel reads: q [B, N, H, 128] raw, wq [128],
    k / v [B or 1, n, H, 128], c [B, N, H * 128] (or what broadcasts to it) = ip_scale * row weight * gate, absent factors 1.
        qh = bf16(q rsqrt(mean(q^2) + eps) wq)        rounded HERE as the kernel rounds its first product's operand
        p  = softmax(qh k^T sm_scale),   term = c p v
    Returns (term, pv, E_s): pv = |c| sum_j p_j |v_j| [B, N, H * 128], what the bf16 rounding of P is relative to, and E_s [B, N, H] =
    136 x 2^-24 sm_scale max_j sum_d |qh_d k_jd|: the fp32 error of a 128-term score summed in any order (128), the subtraction of the
    maximum and the product with the scale (8 more)."""
    B, N, H, Dh = q.shape
    qh, _ = bf16_round64(ip_qhat64(q, wq, eps))
    kd, vd = k.double().expand(B, -1, -1, -1), v.double().expand(B, -1, -1, -1)
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", qh, kd) * sm_scale, dim=-1)
    o = torch.einsum("bhqk,bkhd->bqhd", p, vd).reshape(B, N, H * Dh)
    oa = torch.einsum("bhqk,bkhd->bqhd", p, vd.abs()).reshape(B, N, H * Dh)
    c = c.double()
    e_s = 136 * U24 * sm_scale * torch.einsum("bqhd,bkhd->bhqk", qh.abs(), kd.abs()).amax(-1).permute(0, 2, 1)
    return c * o, c.abs() * oa, e_s.contiguous()


# ------------------------------------------------------------------------------------------------ token passes and e4m3 producers
FP8 = torch.float8_e4m3fn
NAN_U8 = 0x7F                    # an e4m3 NaN: what a byte the kernel must not read, or failed to write, holds
U24, U23 = 2.0 ** -24, 2.0 ** -23   # one fp32 rounding (half an ulp, relative); one fp32 ulp


def guarded3(vals, pad_rows, ld, fill, dtype, device="cpu"):
    """[B, R + pad_rows, ld] holding `fill`, with vals [B, R, D] at [:, :R, :D]: row stride ld > D and a padded batch stride.
    Returns (buffer, the [B, R, D] view)."""
    B, R, D = vals.shape
    buf = torch.full((B, R + pad_rows, ld), fill, dtype=dtype)
    buf[:, :R, :D] = vals.to(dtype)
    buf = buf.to(device)
    return buf, buf[:, :R, :D]


def outside3_is(buf, R, D, fill):
    """True when everything of the 3-D buffer outside [:, :R, :D] still holds `fill` exactly."""
    m = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    m[:, :R, :D] = False
    rest = buf[m]
    return same_bits(rest, torch.full_like(rest, fill))


def ulp_e4m3(t):
    """The spacing of the e4m3 grid at t (fp64): 2^(max(floor(log2 |t|), -6) - 3). Three mantissa bits; below 2^-6 the grid is the
    subnormal one, spacing 2^-9 (also at 0)."""
    a = t.double().abs().clamp_min(2.0 ** -6)
    return torch.exp2(torch.floor(torch.log2(a)).clamp_min(-6.0) - 3.0)


def e4m3_finite(q):
    """True when no byte of the e4m3 tensor is a NaN pattern (0x7f / 0xff); e4m3fn has no infinity, so every other byte is
    finite with |value| <= 448."""
    return not bool(((q.view(torch.uint8) & 0x7F) == 0x7F).any())


def fold_zero(b):
    """e4m3 bytes with -0 (0x80) folded onto +0."""
    b = b.view(torch.uint8)
    return torch.where(b == 0x80, torch.zeros_like(b), b)


def ln_depth(D):
    """Additions an element's value goes through in layernorm_mod_kernel's row sums: a lane adds the 8 values of each of its chunks
    in sequence (at most ceil(D / 512) chunks hold columns < D for a lane), then six butterfly levels, then the division by D, and
    one more for the product or subtraction that made the addend. D / 64 + 8 where D is a multiple of 512."""
    return 8 * ((D + 511) // 512) + 8


def layernorm_ref(x, shift, scale, eps=1e-6, mean_div=None):
    """fp64 LayerNorm (no affine, biased variance) + modulation of x [B, R, D] with shift / scale [B, D] or None:
        y = (x - mean) rstd (1 + scale) + shift.
    Returns (y, by): by bounds the kernel's fp32 evaluation of the element (everything but the rounding of the output), to first
    order, with u = 2^-24 and k = ln_depth(D):
      em = k u mean|x|                                      the row mean (summation depth k, relative to the sum of |x|)
      ev = (k + 4) u var + 2 em mean|x - mean| + em^2       the variance: its own sum, the squares of d = x - mean each carrying
                                                            em + u |d|
      er = rstd (ev / (2 (var + eps)) + 2 u + 2^-22)        rsqrtf(var / D + eps): its argument's error halved, the division and
                                                            the sum with eps, and 2 ulp for the device's rsqrtf (its documented
                                                            accuracy is 1 ulp)
      by = ((em + u |d|) rstd + |d| er) |1 + scale| + 8 u (|d| rstd |1 + scale| + |shift|)
    the last term the element's own operations (subtraction, two products, 1 + scale, the sum with shift).
    mean_div: divide the row sum by this instead of D — a deliberately wrong reference for the tests of the bound itself."""
    xd = x.double()
    D = xd.shape[-1]
    mean = xd.sum(-1, keepdim=True) / (D if mean_div is None else mean_div)
    d = xd - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    s1 = torch.ones(xd.shape[0], 1, D, dtype=F64) if scale is None else 1.0 + scale.double()[:, None, :]
    sh = torch.zeros(xd.shape[0], 1, D, dtype=F64) if shift is None else shift.double()[:, None, :]
    y = d * rstd * s1 + sh
    k = ln_depth(D)
    em = k * U24 * xd.abs().mean(-1, keepdim=True)
    ev = (k + 4) * U24 * var + 2 * em * d.abs().mean(-1, keepdim=True) + em * em
    er = rstd * (ev / (2 * (var + eps)) + 2 * U24 + 2.0 ** -22)
    by = ((em + U24 * d.abs()) * rstd + d.abs() * er) * s1.abs() + 8 * U24 * (d.abs() * rstd * s1.abs() + sh.abs())
    return y, by


def ln_case(B, R, D, dtype, seed):
    """Data of one LayerNorm case, on the CPU: x [B, R, D] in `dtype` (rows 3 randn + 0.5; row (0, 1) = 100 + randn, where a
    one-pass variance fails; row (0, 3) constant, variance 0; row (1, 2) randn with one element 50 in the last 8 columns), and the
    modulation table [B, 2 D + 8] fp32, NaN except shift at columns 4 .. 4 + D and scale behind it (chunk views, mod_ld != D).
    Returns (x, table, shift view, scale view)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, R, D, generator=g) * 3 + 0.5
    x[0, 1] = 100 + torch.randn(D, generator=g)
    x[0, 3] = 1.7
    x[1, 2] = torch.randn(D, generator=g)
    x[1, 2, D - 3] = 50.0
    table = torch.full((B, 2 * D + 8), NAN, dtype=F32)
    table[:, 4 : 4 + D] = torch.randn(B, D, generator=g)
    table[:, 4 + D : 4 + 2 * D] = torch.randn(B, D, generator=g) * 0.5
    return x.to(dtype), table, table[:, 4 : 4 + D], table[:, 4 + D : 4 + 2 * D]


# rt_qk_norm_rope8, in units of 2^-23 relative to |a cos| + |b sin| (a, b the pair's normalised values): the sum of 128 squares is 8
# sequential + 4 butterfly additions of rounded products, 13 roundings of 2^-24 on a sum of positive terms; the fma with eps one
# more; rsqrt halves that relative error: 7 x 2^-24. Two multiplications per value (by r, by the weight): 2 x 2^-24. The rotation:
# the inner product, the fma and the other operand's share: 3 x 2^-24. 12 x 2^-24 = 6 x 2^-23. The device rsqrtf's own error is
# not in this count.
QK_COUNTED = 6.0


def qk_norm_rope_ref(x, w_txt, w_img, T, cos, sin, eps=1e-6, txt_rows=None):
    """fp64 q or k RMSNorm + interleaved-pair RoPE of x [B, S, H, 128] (values as the kernel reads them): rows s < T with w_txt, the
    others with w_img; n = x rsqrt(mean(x^2) + eps) w; pair (n0, n1) -> (n0 c - n1 s, n1 c + n0 s) with the row's cos / sin [S, 128].
    Returns (ref, mag): mag = |a cos| + |b sin| of the element, what the fp32 evaluation's error is relative to.
    txt_rows: rows < txt_rows take the text weights instead of rows < T — a deliberately wrong reference for the tests of the bound."""
    xd = x.double()
    B, S, H, Dh = xd.shape
    tr = T if txt_rows is None else txt_rows
    w = torch.empty(S, Dh, dtype=F64)
    if tr > 0:
        w[:tr] = w_txt.double()
    w[tr:] = w_img.double()
    n = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps) * w[None, :, None, :]
    c, s = cos.double()[None, :, None, :], sin.double()[None, :, None, :]
    pr = n.reshape(B, S, H, Dh // 2, 2)
    n0, n1 = pr[..., 0], pr[..., 1]
    cp, sp = c.reshape(1, S, 1, Dh // 2, 2), s.reshape(1, S, 1, Dh // 2, 2)
    ref = torch.stack([n0 * cp[..., 0] - n1 * sp[..., 0], n1 * cp[..., 1] + n0 * sp[..., 1]], dim=-1).reshape(B, S, H, Dh)
    mag = torch.stack([(n0 * cp[..., 0]).abs() + (n1 * sp[..., 0]).abs(), (n1 * cp[..., 1]).abs() + (n0 * sp[..., 1]).abs()],
                      dim=-1).reshape(B, S, H, Dh)
    return ref, mag


QK_EPS = 1e-6


def _orc():
    from oracle import flux_oracle

    return flux_oracle


def qk_weights(seed):
    """bf16 norm weights far apart — wq_txt ~ 1, wk_txt ~ -0.5, wq_img ~ 2, wk_img ~ -1.5, each +- 0.1 — so that a row normalised
    with the wrong set is off by O(1) at its own element."""
    g = torch.Generator().manual_seed(seed)
    return [(c + 0.1 * torch.randn(128, generator=g)).to(BF16) for c in (1.0, -0.5, 2.0, -1.5)]


def qk_tables(S, T, pos0=0):
    """cos / sin [S, 128] from the oracle's rope_table on real ids: text rows at id 0, image rows from latent_image_ids (+ pos0 on
    both axes, so that the angles are not small)."""
    n = S - T
    img = _orc().latent_image_ids(2 * 10, 2 * ((n + 9) // 10))[:n] if n > 0 else torch.zeros(0, 3)
    img = img.clone()
    img[:, 1:] += pos0
    return _orc().rope_table(torch.cat([torch.zeros(T, 3), img], dim=0))


def qk_layout(single, d):
    """(q_off, k_off, ld): the double blocks' q | k | v buffer, or the single blocks' k | v | q | mlp one."""
    return (2 * d, 0, 7 * d + 8) if single else (0, d, 3 * d + 8)


def quant_rows_rule(x, skip_cols=None):
    """The row-quantisation rule in the kernel's own fp32 arithmetic on the CPU, x [rows, D] (values as the kernel reads them):
    scale = fp32(amax * fp32(1 / 448)), 1.0 for an all-zero row; q = e4m3(clamp(x * fp32(1 / scale), +-448)), round to nearest even.
    The clamp comes first: torch's CPU cast gives NaN above 464. Returns (q e4m3, scale fp32).
    skip_cols = (c0, c1): those columns are left out of the row maximum — a deliberately wrong rule for the tests of the checks."""
    x = x.float()
    a = x.abs()
    if skip_cols is not None:
        a = a.clone()
        a[:, skip_cols[0] : skip_cols[1]] = 0
    amax = a.amax(dim=1)
    sc = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    y = (x * (1.0 / sc)[:, None]).clamp(-448.0, 448.0)
    return y.to(FP8), sc


def check_quant_rows(what, q, scale, x):
    """q e4m3 [rows, D] and scale fp32 [rows] from a row quantiser against x [rows, D] (values as read). Every byte finite, and with
    t = x / scale in fp64:
        |q - t| <= ulp_e4m3(t) / 2 + 2^-21 |t|
    the first term the rounding to the e4m3 grid, the second the fp32 reciprocal and product (three roundings, one of them possibly
    a whole ulp). t is not clamped: with the right scale it passes 448 by the second term at most, and a row maximum the scale
    missed shows as |t| far above 448 against a saturated byte."""
    assert e4m3_finite(q), f"{what}: NaN byte"
    qv = q.float().double()
    t = x.double() / scale.double()[:, None]
    return check_bound(what, qv, t, 0.5 * ulp_e4m3(t) + 2.0 ** -21 * t.abs())


def vt8_key_order():
    """Key (inside a 64-key tile) at each of the 64 positions of a row of the e4m3 V^T, from the layout comment at the top of
    csrc/attention_fp8.hip: position p = 32 hh + 16 kt + 4 g + e holds key 32 kt + 8 g + 4 hh + e."""
    key = torch.empty(64, dtype=torch.long)
    for hh in range(2):
        for kt in range(2):
            for g in range(4):
                for e in range(4):
                    key[32 * hh + 16 * kt + 4 * g + e] = 32 * kt + 8 * g + 4 * hh + e
    return key


def vt8_expected(v, swap=None):
    """uint8 [B, H, 128, S64] (S64 = S rounded up to 64): byte [b][h][dd][64 t + p] = e4m3(clamp(v[b][64 t + key(p)][h][dd], +-448)),
    zero for keys >= S. v [B, S, H, 128], values as the kernel reads them. -0 folded onto +0.
    swap = (p0, p1): those two positions of every tile exchanged — a deliberately wrong layout for the tests of the comparison."""
    B, S, H, Dh = v.shape
    S64 = (S + 63) // 64 * 64
    v8 = torch.zeros(B, S64, H, Dh, dtype=torch.uint8)
    v8[:, :S] = v.float().clamp(-448.0, 448.0).to(FP8).view(torch.uint8)
    order = vt8_key_order()
    if swap is not None:
        order = order.clone()
        order[[swap[0], swap[1]]] = order[[swap[1], swap[0]]]
    idx = (torch.arange(S64 // 64)[:, None] * 64 + order[None, :]).reshape(-1)
    return fold_zero(v8[:, idx].permute(0, 2, 3, 1).contiguous())
