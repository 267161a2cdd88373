"""What the tests of tests/test_support_kernels_gpu.py, test_gemm_epilogue_gpu.py, test_attention_edges_gpu.py and test_vae_kernels_gpu.py
share: the fp64 references of the GEMM epilogue, of the convolution and of attention, the per-element bound check, guarded buffers (NaN where a kernel must not read, a sentinel where it must
not write), the bf16 error bound, ulp distances and the run-twice check. A plain helper module, not a test file."""
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
    """fp64 softmax(q k^T scale) v of CPU tensors [B, S, H, Dh] holding exactly the values the kernel reads. Returns (ref, pv) as
    [B, S, H * Dh]: the value and sum_j p_j |v_j| with p the fp64 softmax row — what the bf16 rounding of P (the second product's
    operand) and of the normaliser is relative to."""
    q, k, v = q.double(), k.double(), v.double()
    B, S, H, Dh = q.shape
    sc = Dh ** -0.5 if scale is None else float(scale)
    ref, pv = torch.empty(B, S, H, Dh, dtype=F64), torch.empty(B, S, H, Dh, dtype=F64)
    for b in range(B):
        for h in range(H):                     # one [S, S] matrix at a time
            p = torch.softmax(q[b, :, h] @ k[b, :, h].t() * sc, dim=-1)
            ref[b, :, h], pv[b, :, h] = p @ v[b, :, h], p @ v[b, :, h].abs()
    return ref.reshape(B, S, H * Dh), pv.reshape(B, S, H * Dh)
