"""What the tests of tests/test_support_kernels_gpu.py share: guarded buffers (NaN where a kernel must not read, a sentinel where it must
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
