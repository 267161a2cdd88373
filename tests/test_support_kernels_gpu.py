"""Direct fp64 references for the kernels around the denoising hot path: GroupNorm(+SiLU) and the image / layout kernels of the VAE
(csrc/vae.hip), the prompt encoders' small kernels (csrc/text_encoder.hip) and the elementwise kernels of csrc/norm_elem.hip.

Every test seeds its inputs on the CPU, rounds them to the dtype the kernel reads and compares with plain torch in fp64 on those
values. Memory a kernel must not read holds NaN, memory it must not write holds a sentinel that is checked afterwards, every kernel
runs twice and must give the same bits. The bound for a bf16 output is BF16(ref, slack): |got - ref| <= 2^-8 |ref| + slack, plus
rel-L2 < 3e-3 (tests/support_kernels.py: check_bf16, which prints the measured figures; run with -s to see them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402

import support_kernels as sk  # noqa: E402
from support_kernels import BF16, F32, NAN, SENT, SENT_U8  # noqa: E402

RT_E_SHAPE = -3


@pytest.fixture(scope="module")
def lib(gpu):
    from reptext_amd import native

    return native.load()


@pytest.fixture(scope="module")
def ops(gpu):
    from reptext_amd import ops as _ops

    return _ops


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(code):
    assert code == 0, f"native call returned {code}"


def _f32(v):
    """The value a float argument of the C ABI has once it is a C float."""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------------------------------------------------------ GroupNorm (+SiLU)
# (C, H, W, B, G, reference on the device): the smallest shapes that reach each path of gn_stats / gn_reduce / gn_apply
GN_CASES = {
    "ppb32_ragged_b2": (64, 12, 20, 2, 32, False),       # one pixel per thread, last block of 16 with idle threads, two batch entries
    "pstep4_unroll_and_tail": (512, 7, 8, 1, 32, False),  # last block of 24: one unrolled trip and two remainder trips
    "pstep4_two_unrolled": (512, 16, 16, 1, 32, False),   # 8 pixels per thread: two unrolled trips, no remainder
    "ppb64_nblk600": (256, 192, 200, 1, 32, False),       # 600 blocks of 64 pixels: the reduce walks more partials than it has segments
    "ppb128_ragged": (128, 264, 264, 1, 32, False),       # 545 blocks of 128, last one of 64
    "ppb256_four_unrolled": (128, 512, 512, 1, 32, True),  # 16 pixels per thread: four unrolled trips
    "group_spans_chunks": (64, 12, 20, 1, 4, False),      # cpg = 16: a group spans two 8-channel chunks
}
# (pixels per block, blocks, pixels of the last block, pixel step = 256 / (C/8)) each case is there for. A guard on the case table
# only: it is checked against support_kernels.gn_pix_per_block, a Python copy, so it does not notice a change to the C++ function;
# whoever changes that re-derives these shapes.
GN_PATH = {
    "ppb32_ragged_b2": (32, 8, 16, 32), "pstep4_unroll_and_tail": (32, 2, 24, 4), "pstep4_two_unrolled": (32, 8, 32, 4),
    "ppb64_nblk600": (64, 600, 64, 8), "ppb128_ragged": (128, 545, 64, 16), "ppb256_four_unrolled": (256, 1024, 256, 16),
    "group_spans_chunks": (32, 8, 16, 32),
}


def _gn_workspace(lib, B, H, W, G, device):
    return torch.full((int(lib.rt_groupnorm_ws_bytes(B, H, W, G)),), 0xFF, dtype=torch.uint8, device=device)   # stale bytes would be NaN


def _gn_launch(lib, xh, y, gamma, beta, B, H, W, C, G, eps, silu, ws=None):
    if ws is None:
        ws = _gn_workspace(lib, B, H, W, G, xh.device)
    code = lib.rt_groupnorm_silu_nhwc(xh.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws.data_ptr(), B, H, W, C, G, eps,
                                      silu, _st())
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize("name", list(GN_CASES))
def test_groupnorm_silu(lib, gpu, name):
    """rt_groupnorm_silu_nhwc against fp64 GroupNorm on activations whose mean is 8 standard deviations from zero (what the variance as
    E[x²] - mean² from fp32 partials has to survive): BF16(ref, 2e-5), rel-L2 < 3e-3, halo and input untouched, bitwise repeatable,
    and a batch entry gives the bits of its own B = 1 launch."""
    C, H, W, B, G, on_device = GN_CASES[name]
    ppb = sk.gn_pix_per_block(H * W)
    nblk = -(-H * W // ppb)
    assert (ppb, nblk, H * W - (nblk - 1) * ppb, 256 // (C // 8)) == GN_PATH[name]
    eps = 1e-6
    g = torch.Generator().manual_seed(1000 + list(GN_CASES).index(name))
    gain = 0.25 * 16.0 ** torch.rand(C, generator=g)                      # per channel, in [0.25, 4]
    offs = torch.stack([8.0 * gain * (1.0 - 1.5 * b) for b in range(B)])    # 8 standard deviations; entry 1: -4, another offset
    x = (torch.randn(B, H, W, C, generator=g) * gain + offs[:, None, None, :]).to(BF16)
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).to(BF16)
    beta = (0.5 * torch.randn(C, generator=g)).to(BF16)
    dev = gpu if on_device else torch.device("cpu")
    ref = sk.groupnorm_ref(x.to(dev), gamma.to(dev), beta.to(dev), G, _f32(eps))
    xh = sk.haloed(x, NAN, device=gpu)
    xh0 = xh.clone()
    dgamma, dbeta = gamma.to(gpu), beta.to(gpu)                            # kept alive across the raw-pointer calls
    for silu in (0, 1):
        def run():
            y = sk.haloed((B, H, W, C), SENT, device=gpu)
            _ok(_gn_launch(lib, xh, y, dgamma, dbeta, B, H, W, C, G, eps, silu))
            return y
        y = sk.twice(run)
        assert sk.halo_is(y, SENT), "output halo written"
        assert sk.same_bits(xh, xh0), "input modified"
        sk.check_bf16(f"groupnorm {name} silu={silu}", y[:, 1:-1, 1:-1, :].to(dev), ref[silu], 2e-5)
        if B > 1:
            for b in range(B):
                y1 = sk.haloed((1, H, W, C), SENT, device=gpu)
                xb = xh[b:b + 1].contiguous()
                _ok(_gn_launch(lib, xb, y1, dgamma, dbeta, 1, H, W, C, G, eps, silu))
                assert sk.same_bits(y1[0], y[b]), f"batch entry {b} differs from its own B = 1 launch"


@pytest.mark.parametrize("C,H,W,B,G", [(1024, 4, 4, 1, 1024), (8, 65536, 1, 1, 1)])
def test_groupnorm_refuses_before_it_launches(lib, gpu, C, H, W, B, G):
    """2·G > 1024 (the reduce's workgroup) and B·H > 65535 (the apply grid) are RT_E_SHAPE, and nothing has been queued by then: after
    a synchronize the workspace still holds the 0xFF it was filled with (the statistics and reduce kernels, the ones a late check
    lets through, write only there) and the output still holds the sentinel. Real, correctly sized buffers."""
    g = torch.Generator().manual_seed(7)
    xh = sk.haloed(torch.randn(B, H, W, C, generator=g), NAN, device=gpu)
    y = sk.haloed((B, H, W, C), SENT, device=gpu)
    gamma, beta = torch.ones(C, dtype=BF16, device=gpu), torch.zeros(C, dtype=BF16, device=gpu)
    ws = _gn_workspace(lib, B, H, W, G, gpu)
    assert ws.numel() > 0
    assert _gn_launch(lib, xh, y, gamma, beta, B, H, W, C, G, 1e-6, 1, ws=ws) == RT_E_SHAPE
    assert bool((ws == 0xFF).all()), "the workspace was written: kernels were queued before the call was refused"
    assert sk.same_bits(y, torch.full_like(y, SENT)), "the output was written by a refused call"


# ------------------------------------------------------------------------------------------------------------------- rt_rmsnorm_rows
def _rmsnorm_ref(x, w, eps):
    xd = x.double()
    return xd * torch.rsqrt((xd * xd).mean(dim=-1, keepdim=True) + eps) * w.double()


@pytest.mark.parametrize("x_f32", [0, 1])
@pytest.mark.parametrize("D", [8, 128, 256, 520, 4096])
def test_rmsnorm_rows(lib, gpu, D, x_f32):
    """T5LayerNorm rows against fp64: D up to 4096 (eight trips of the 512-column loop; at 520 the second trip is live on lane 0 only),
    ragged 4-row groups, both input types, ldx = D + 8 and ldo = D + 16, one row around 1e-3 (eps matters) and one around 1e3.
    BF16(ref, 1e-6·max|ref|)."""
    eps = 1e-6
    g = torch.Generator().manual_seed(20 + D + x_f32)
    w = (1.0 + 0.2 * torch.randn(D, generator=g)).to(BF16)
    dw = w.to(gpu)
    for rows in (1, 5, 9):
        x = torch.randn(rows, D, generator=g)
        x[0] *= 1e-3
        if rows > 1:
            x[rows - 1] *= 1e3                        # the last row of a ragged group
        x = x if x_f32 else x.to(BF16)
        ref = _rmsnorm_ref(x, w, _f32(eps))
        dx = sk.guarded_rows(x, D + 8, 2, NAN, F32 if x_f32 else BF16, gpu)

        def run():
            out = torch.full((rows + 2, D + 16), SENT, dtype=BF16, device=gpu)
            _ok(lib.rt_rmsnorm_rows(dx.data_ptr(), D + 8, x_f32, dw.data_ptr(), out.data_ptr(), D + 16, rows, D, eps, _st()))
            torch.cuda.synchronize()
            return out
        out = sk.twice(run)
        assert sk.outside_is(out, rows, D, SENT), "wrote outside [rows, D]"
        sk.check_bf16(f"rmsnorm D={D} rows={rows} f32={x_f32}", out[:rows, :D].cpu(), ref, 1e-6 * float(ref.abs().max()))


def test_rmsnorm_heads(ops, gpu):
    """ops.rmsnorm_heads_ (the IP-Adapter's weightless K norm): 48 groups of 128 fp32 values, weight of ones."""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 3, 8, 128, generator=g) * (0.05 + 4.0 * torch.rand(2, 3, 8, 1, generator=g))
    eps = 1e-5
    ref = _rmsnorm_ref(x, torch.ones(128), _f32(eps))
    dx, ones = x.to(gpu), torch.ones(128, dtype=BF16, device=gpu)
    out = sk.twice(lambda: ops.rmsnorm_heads_(dx, torch.full(x.shape, SENT, dtype=BF16, device=gpu), ones, eps))
    assert sk.same_bits(dx.cpu(), x)
    sk.check_bf16("rmsnorm_heads_", out.cpu(), ref, 1e-6 * float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------------------------------- softmaxes
def _softmax_ref(z):
    p = torch.softmax(z.double(), dim=-1)
    return torch.where(torch.isnan(p), torch.zeros_like(p), p)          # a fully masked row is all zeros by contract


@pytest.mark.parametrize("bias_kind", ["none", "dense", "causal", "masked_row"])
@pytest.mark.parametrize("cols,cols_out,ld", [(77, 128, 128), (512, 512, 512), (300, 320, 384), (1, 64, 64)])
def test_softmax_rows_bias(lib, gpu, cols, cols_out, ld, bias_kind):
    """softmax(scale·s + bias) rows against fp64 up to the pipeline's T = 512 (two trips of the 256-thread loops), with no bias, a dense
    one, a causal -inf mask and one fully masked row (exactly zero). Scores and biases at columns >= cols are NaN and must not reach
    the output; columns cols..cols_out-1 are exactly zero; columns >= cols_out and the rows behind keep the sentinel.
    BF16(ref, 1e-7), |row sum - 1| < 4e-3."""
    rows = 6
    g = torch.Generator().manual_seed(cols * 7 + len(bias_kind))
    for scale, gain in ((0.125, 8.0), (1.0, 8.0)):
        s = torch.randn(rows, cols, generator=g) * gain
        bias = None
        if bias_kind != "none":
            bias = torch.randn(rows, cols, generator=g)
        if bias_kind == "causal":
            keep = torch.arange(cols)[None, :] <= (torch.arange(rows)[:, None] * max(cols // rows, 1))
            bias = torch.where(keep, torch.zeros(()), torch.full((), float("-inf")))
        if bias_kind == "masked_row":
            bias[2] = float("-inf")
        z = s.double() * scale + (bias.double() if bias is not None else 0.0)
        ref = _softmax_ref(z)
        ds = sk.guarded_rows(s, ld, 1, NAN, F32, gpu)
        db = sk.guarded_rows(bias, ld, 1, NAN, F32, gpu) if bias is not None else None

        def run():
            p = torch.full((rows + 1, ld), SENT, dtype=BF16, device=gpu)
            _ok(lib.rt_softmax_rows_bias(ds.data_ptr(), ld, db.data_ptr() if db is not None else None, ld, p.data_ptr(), ld, rows, cols,
                                         cols_out, scale, _st()))
            torch.cuda.synchronize()
            return p
        p = sk.twice(run).cpu()
        assert sk.outside_is(p, rows, cols_out, SENT), "wrote outside [rows, cols_out]"
        assert sk.same_bits(p[:rows, cols:cols_out], torch.zeros(rows, cols_out - cols, dtype=BF16)), "K padding is not exactly zero"
        got = p[:rows, :cols]
        sk.check_bf16(f"softmax_rows_bias {cols}/{cols_out}/{ld} {bias_kind} scale={scale}", got, ref, 1e-7)
        sums = got.double().sum(dim=1)
        live = torch.ones(rows, dtype=torch.bool)
        if bias_kind == "masked_row":
            live[2] = False
            assert sk.same_bits(got[2], torch.zeros(cols, dtype=BF16)), "fully masked row is not exactly zero"
        assert float((sums[live] - 1.0).abs().max()) < 4e-3


@pytest.mark.parametrize("cols", [4, 1028, 4096])
def test_softmax_rows(lib, gpu, cols):
    """rt_softmax_rows (f32 scores -> bf16, four columns per thread: one lane at cols = 4, a ragged second trip at 1028, four trips at
    4096) against fp64. BF16(ref, 1e-7)."""
    rows, scale = 3, 0.125
    g = torch.Generator().manual_seed(cols)
    s = torch.randn(rows, cols, generator=g) * 8.0
    ref = _softmax_ref(s.double() * scale)
    ds = sk.guarded_rows(s, cols, 1, NAN, F32, gpu)

    def run():
        p = torch.full((rows + 1, cols), SENT, dtype=BF16, device=gpu)
        _ok(lib.rt_softmax_rows(ds.data_ptr(), p.data_ptr(), rows, cols, scale, _st()))
        torch.cuda.synchronize()
        return p
    p = sk.twice(run).cpu()
    assert sk.outside_is(p, rows, cols, SENT)
    sk.check_bf16(f"softmax_rows cols={cols}", p[:rows], ref, 1e-7)
    assert float((p[:rows].double().sum(dim=1) - 1.0).abs().max()) < 4e-3


# ------------------------------------------------------------------------------------ transpose, gated product, quick-GELU, gather
@pytest.mark.parametrize("R,C", [(64, 64), (70, 64), (128, 64), (100, 130)])
def test_transpose_bf16(lib, gpu, R, C):
    """out[c][r] = in[r][c] on a ramp of distinct bf16 values, ld_in = C + 8 and ld_out = R + 6: bit-exact, padding untouched."""
    ramp = (torch.arange(R * C, dtype=torch.int32) + 0x0100).to(torch.int16).view(BF16).reshape(R, C)   # distinct positive normals
    assert int(ramp.view(torch.int16).max()) < 0x7F80
    din = sk.guarded_rows(ramp, C + 8, 1, NAN, BF16, gpu)

    def run():
        out = torch.full((C + 1, R + 6), SENT, dtype=BF16, device=gpu)
        _ok(lib.rt_transpose_bf16(din.data_ptr(), out.data_ptr(), R, C, C + 8, R + 6, _st()))
        torch.cuda.synchronize()
        return out
    out = sk.twice(run).cpu()
    assert sk.outside_is(out, C, R, SENT)
    assert sk.same_bits(out[:C, :R], ramp.t().contiguous())


@pytest.mark.parametrize("F", [8, 640, 10240])
def test_gated_mul(lib, gpu, F):
    """out[r][c] = bf16(x[r][c] · x[r][F + c]), ldx = 2F + 8, ldo = F + 8: one fp32 product and one rounding, so bit-exact."""
    rows = 3
    g = torch.Generator().manual_seed(F)
    x = torch.randn(rows, 2 * F, generator=g).to(BF16)
    ref = (x[:, :F].float() * x[:, F:].float()).to(BF16)
    dx = sk.guarded_rows(x, 2 * F + 8, 1, NAN, BF16, gpu)

    def run():
        out = torch.full((rows + 1, F + 8), SENT, dtype=BF16, device=gpu)
        _ok(lib.rt_gated_mul(dx.data_ptr(), 2 * F + 8, out.data_ptr(), F + 8, rows, F, _st()))
        torch.cuda.synchronize()
        return out
    out = sk.twice(run).cpu()
    assert sk.outside_is(out, rows, F, SENT)
    assert sk.same_bits(out[:rows, :F], ref)


@pytest.mark.parametrize("n", [8, 8000])
def test_quick_gelu(lib, gpu, n):
    """x·sigmoid(1.702x) in place against fp64, with 0, ±60 (exp overflows one way, vanishes the other) and a randn·3 body; the eight
    elements behind n keep the sentinel. BF16(ref, 1e-6)."""
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * 3.0).to(BF16)
    x[:3] = torch.tensor([0.0, 60.0, -60.0], dtype=BF16)
    ref = x.double() * torch.sigmoid(1.702 * x.double())
    full = torch.cat([x, torch.full((8,), SENT, dtype=BF16)])

    def run():
        d = full.to(gpu)
        _ok(lib.rt_quick_gelu(d.data_ptr(), n, _st()))
        torch.cuda.synchronize()
        return d
    out = sk.twice(run).cpu()
    assert sk.same_bits(out[n:], full[n:])
    sk.check_bf16(f"quick_gelu n={n}", out[:n], ref, 1e-6)


@pytest.mark.parametrize("D", [8, 264])
def test_embedding_gather(lib, gpu, D):
    """Rows of a bf16 table by id, ld = D + 8 and ldo = D + 16, with ids 0, vocab-1, a repeat and the out-of-range -3 and vocab+5, which
    the kernel clamps to the first and last row (the encoders rely on it). The table sits between NaN rows, so an unclamped or
    off-by-one id shows. Bit-exact."""
    vocab, lead = 50, 4
    g = torch.Generator().manual_seed(D)
    table = torch.randn(vocab, D, generator=g).to(BF16)
    whole = torch.full((lead + vocab + 8, D + 8), NAN, dtype=BF16)
    whole[lead:lead + vocab, :D] = table
    dwhole = whole.to(gpu)
    ids = torch.tensor([0, vocab - 1, 7, 7, -3, vocab + 5, 23], dtype=torch.int32)
    dids = ids.to(gpu)
    n = ids.numel()
    ref = table[ids.clamp(0, vocab - 1).long()]

    def run():
        out = torch.full((n + 1, D + 16), SENT, dtype=BF16, device=gpu)
        _ok(lib.rt_embedding_gather(dwhole[lead:].data_ptr(), D + 8, dids.data_ptr(), out.data_ptr(), D + 16, n, D, vocab, _st()))
        torch.cuda.synchronize()
        return out
    out = sk.twice(run).cpu()
    assert sk.outside_is(out, n, D, SENT)
    assert sk.same_bits(out[:n, :D], ref)


# ------------------------------------------------------------------------------------------------------ image tail and layout kernels
IMG = dict(B=2, C=3, Cp=4, H=6, W=10)


def test_image_out(lib, gpu):
    """Decoder tail: haloed NHWC f32 (pad channel and halo NaN) -> NCHW f32, bit-exact, and uint8 HWC that EQUALS
    round(clamp(x/2 + 0.5, 0, 1)·255) in fp32 (round to nearest even; x·0.5 is exact, so a fused multiply-add changes nothing), with
    exact -1, 0, 1 and the half-way points (2k+1)/255 - 1 among the inputs. Both outputs together and each alone."""
    B, C, Cp, H, W = (IMG[k] for k in ("B", "C", "Cp", "H", "W"))
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, H, W, C, generator=g) * 2.6 - 1.3
    ks = torch.tensor([0, 1, 2, 63, 64, 127, 128, 200, 253, 254], dtype=F32)
    special = torch.cat([torch.tensor([-1.0, 0.0, 1.0]), (2 * ks + 1) / 255 - 1])
    x.view(-1)[:special.numel()] = special
    x.view(-1)[-special.numel():] = special
    ref_u8 = torch.round((x * 0.5 + 0.5).clamp(0, 1) * 255).to(torch.uint8)            # [B, H, W, C], fp32 on the CPU
    ref_nchw = x.permute(0, 3, 1, 2).contiguous()
    dx = sk.haloed(x, NAN, Cp=Cp, dtype=F32, device=gpu)
    n = B * C * H * W
    for want_nchw, want_u8 in ((1, 1), (1, 0), (0, 1)):
        def run():
            nchw = torch.full((n + 8,), SENT, dtype=F32, device=gpu)
            u8 = torch.full((n + 8,), SENT_U8, dtype=torch.uint8, device=gpu)
            _ok(lib.rt_image_out(dx.data_ptr(), nchw.data_ptr() if want_nchw else None, u8.data_ptr() if want_u8 else None, B, H, W, Cp, C, _st()))
            torch.cuda.synchronize()
            return nchw, u8
        nchw, u8 = (t.cpu() for t in sk.twice(run))
        assert sk.same_bits(nchw[n:], torch.full((8,), SENT)) and sk.same_bits(u8[n:], torch.full((8,), SENT_U8, dtype=torch.uint8))
        if want_nchw:
            assert sk.same_bits(nchw[:n].reshape(B, C, H, W), ref_nchw)
        else:
            assert sk.same_bits(nchw, torch.full((n + 8,), SENT)), "nchw written though not requested"
        if want_u8:
            got = u8[:n].reshape(B, H, W, C)
            diff = (got.int() - ref_u8.int()).abs()
            print(f"[support] image_out u8 (nchw={want_nchw}): {int((diff != 0).sum())} of {n} differ, max {int(diff.max())}")
            assert torch.equal(got, ref_u8)
        else:
            assert sk.same_bits(u8, torch.full((n + 8,), SENT_U8, dtype=torch.uint8)), "u8 written though not requested"


def test_nchw_haloed_nhwc_round_trip(lib, gpu):
    """rt_nchw_to_haloed_nhwc then rt_haloed_nhwc_to_nchw: the interior is bf16(x) bit for bit, the pad channel exactly zero, the
    destination's halo keeps the sentinel; the way back reads a buffer whose halo and pad channel are NaN."""
    B, C, Cp, H, W = (IMG[k] for k in ("B", "C", "Cp", "H", "W"))
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, C, H, W, generator=g)
    dx = x.to(gpu)
    n = x.numel()

    def run():
        y = sk.haloed((B, H, W, Cp), SENT, device=gpu)
        _ok(lib.rt_nchw_to_haloed_nhwc(dx.data_ptr(), y.data_ptr(), B, C, H, W, Cp, _st()))
        torch.cuda.synchronize()
        return y
    y = sk.twice(run)
    assert sk.halo_is(y, SENT), "halo of the destination written"
    inner = y[:, 1:-1, 1:-1, :].cpu()
    assert sk.same_bits(inner[..., :C], x.permute(0, 2, 3, 1).to(BF16).contiguous())
    assert sk.same_bits(inner[..., C:], torch.zeros(B, H, W, Cp - C, dtype=BF16)), "pad channels are not exactly zero"
    back_in = sk.haloed(inner[..., :C], NAN, Cp=Cp, device=gpu)

    def run_back():
        out = torch.full((n + 8,), SENT, dtype=F32, device=gpu)
        _ok(lib.rt_haloed_nhwc_to_nchw(back_in.data_ptr(), out.data_ptr(), B, C, H, W, Cp, _st()))
        torch.cuda.synchronize()
        return out
    out = sk.twice(run_back).cpu()
    assert sk.same_bits(out[n:], torch.full((8,), SENT))
    assert sk.same_bits(out[:n].reshape(B, C, H, W), x.to(BF16).float())


def test_unpack_latents_haloed(lib, gpu):
    """Packed latents -> haloed NHWC with value·inv_scale + shift: positions as orc.unpack_latents places them (a layout error is O(1)),
    every element within one bf16 ulp of bf16(fp64(v·inv_scale + shift)), pad channels exactly zero, halo untouched."""
    B, C, Cp, H2, W2 = 2, 16, 64, 6, 10
    inv_scale, shift = _f32(1.0 / 0.3611), _f32(0.1159)
    g = torch.Generator().manual_seed(8)
    packed = torch.randn(B, (H2 // 2) * (W2 // 2), 4 * C, generator=g).to(BF16)
    placed = orc.unpack_latents(packed, H2 * 8, W2 * 8)                                  # [B, C, H2, W2], the packed values moved
    assert placed.shape == (B, C, H2, W2)
    ref = (placed.double() * inv_scale + shift).permute(0, 2, 3, 1).contiguous()
    dp = packed.to(gpu)

    def run():
        y = sk.haloed((B, H2, W2, Cp), SENT, device=gpu)
        _ok(lib.rt_unpack_latents_haloed(dp.data_ptr(), y.data_ptr(), B, C, H2, W2, Cp, inv_scale, shift, _st()))
        torch.cuda.synchronize()
        return y
    y = sk.twice(run)
    assert sk.halo_is(y, SENT), "halo written"
    inner = y[:, 1:-1, 1:-1, :].cpu()
    assert sk.same_bits(inner[..., C:], torch.zeros(B, H2, W2, Cp - C, dtype=BF16)), "pad channels are not exactly zero"
    d = sk.ulp_distance(inner[..., :C].contiguous(), ref.to(BF16))
    print(f"[support] unpack_latents_haloed: {d} bf16 ulp from bf16(fp64), max|err| {float((inner[..., :C].double() - ref).abs().max()):.3e}")
    assert d <= 1


# ----------------------------------------------------------------------------------------------------- elementwise (csrc/norm_elem.hip)
GRID_CAP = 4096 * 256            # threads of the largest grid the elementwise kernels launch: more work takes a second grid-stride trip


@pytest.mark.parametrize("n", [8 * 1000 + 5, 8 * GRID_CAP + 8])
def test_euler_step_sizes(ops, gpu, n):
    """x += dsigma·v in bf16 with the scalar tail kernel live (n % 8 = 5) and with a second grid-stride trip (one vector past the grid
    cap): bit-exact against orc.euler_step, as test_euler_pack_cast_mask asserts for its one size. The larger size is also where the
    oracle's two fp32 roundings (product, then sum) can be told from a fused multiply-add: the two differ in about one element in
    two million."""
    g = torch.Generator().manual_seed(n % 1000)
    x = torch.randn(n, generator=g).to(BF16)
    v = torch.randn(n, generator=g).to(BF16)
    ref = orc.euler_step(x, v, 1.0, 1.0 - 0.0116)
    dv = v.to(gpu)
    out = sk.twice(lambda: ops.euler_step_(x.to(gpu), dv, -0.0116)).cpu()
    diff = sk.bits(out) != sk.bits(ref)
    print(f"[support] euler_step_ n={n}: {int(diff.sum())} elements differ from the oracle")
    assert sk.same_bits(out, ref)
    assert sk.same_bits(dv.cpu(), v)


@pytest.mark.parametrize("with_bf16", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 67, 1000, GRID_CAP + 3, 4 * (GRID_CAP + 1000) + 3])
def test_euler_step_f32(ops, gpu, n, with_bf16):
    """fp32 master state x32 += dsigma·v (v bf16): within one fp32 ulp of the fp64 axpy, and the optional bf16 copy is EXACTLY the bf16
    rounding of the x32 that was returned. The kernel takes groups of four elements, then what is left one at a time: no group (1, 3),
    one group (4), a group and a tail (5, 67), and a last size at which a thread takes a second group (the grid-stride trip past the
    grid cap) and three elements are left for the tail."""
    g = torch.Generator().manual_seed(n % 1000 + with_bf16)
    x = torch.randn(n, generator=g)
    v = torch.randn(n, generator=g).to(BF16)
    ds = -0.0116
    ref = x.double() + _f32(ds) * v.double()
    dv = v.to(gpu)

    def run():
        x32 = x.to(gpu)
        xb = torch.full((n,), SENT, dtype=BF16, device=gpu) if with_bf16 else None
        ops.euler_step_f32_(x32, dv, ds, xb)
        return x32, xb
    x32, xb = sk.twice(run)
    x32 = x32.cpu()
    u = sk.f32_ulps_from(x32, ref)
    print(f"[support] euler_step_f32_ n={n} bf16={with_bf16}: {u:.3f} fp32 ulp from the fp64 axpy")
    assert u <= 1.0
    if with_bf16:
        assert sk.same_bits(xb.cpu(), x32.to(BF16))


def _macc_inputs(shape, g, device):
    """y and x share their sign element by element and the row scale is >= 0, so the sum does not cancel: the bound in ulps of the
    result is then the bound of the kernel's three fp32 roundings (alpha·rowscale, the product, the sum) whatever the values."""
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    y = (torch.randn(shape, generator=g).abs() * sign).to(device)
    x = (torch.randn(shape, generator=g).abs() * sign).to(BF16).to(device)
    return y, x


@pytest.mark.parametrize("use_rowscale", [False, True])
@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("y_dtype", [F32, BF16])
def test_masked_accumulate(ops, gpu, y_dtype, accumulate, use_rowscale):
    """y (+)= alpha·rowscale[r]·x on [2, 96, 256] against fp64, fp32 and bf16 destinations, with and without accumulation and row
    scale. fp32 destination: within 2 fp32 ulp (three roundings: alpha·rowscale, the product, the sum; y and x have equal signs so the
    sum does not cancel and an ulp of the result is the right unit). bf16 destination: BF16(ref, 1e-6)."""
    g = torch.Generator().manual_seed(40 + accumulate + 2 * use_rowscale)
    shape, alpha = (2, 96, 256), 0.7
    y, x = _macc_inputs(shape, g, "cpu")
    y = y.to(y_dtype)
    rs = torch.rand(shape[1], generator=g) if use_rowscale else None
    m = (rs.double() if use_rowscale else torch.ones(shape[1], dtype=torch.float64)) * _f32(alpha)
    ref = m[None, :, None] * x.double() + (y.double() if accumulate else 0.0)
    dx, drs = x.to(gpu), (rs.to(gpu) if use_rowscale else None)
    out = sk.twice(lambda: ops.masked_accumulate_(y.to(gpu), dx, drs, alpha=alpha, accumulate=accumulate)).cpu()
    what = f"masked_accumulate_ {y_dtype} acc={accumulate} rowscale={use_rowscale}"
    if y_dtype == F32:
        u = sk.f32_ulps_from(out, ref)
        print(f"[support] {what}: {u:.3f} fp32 ulp from fp64")
        assert u <= 2.0
    else:
        sk.check_bf16(what, out, ref, 1e-6)
    assert sk.same_bits(dx.cpu(), x)


@pytest.mark.parametrize("y_dtype", [F32, BF16])
def test_masked_accumulate_mixed_signs(ops, gpu, y_dtype):
    """The general case: y and alpha·rowscale·x of either sign, so the sum may cancel. The three fp32 roundings are then bounded in ulps
    of the larger operand, not of the result: alpha·rowscale costs up to 1 ulp of the product, the product 0.5 ulp of itself, the sum
    0.5 ulp of a result no larger than max(|y|, |m·x|) where it cancels. fp32 destination: within 2 fp32 ulp of
    max(|y|, |m·x|, |ref|). bf16 destination: BF16(ref, 1e-6)."""
    g = torch.Generator().manual_seed(47)
    shape, alpha = (2, 96, 256), 0.7
    y = torch.randn(shape, generator=g).to(y_dtype)
    x = torch.randn(shape, generator=g).to(BF16)
    rs = torch.rand(shape[1], generator=g)
    prod = (rs.double() * _f32(alpha))[None, :, None] * x.double()
    ref = prod + y.double()
    dx, drs = x.to(gpu), rs.to(gpu)
    out = sk.twice(lambda: ops.masked_accumulate_(y.to(gpu), dx, drs, alpha=alpha, accumulate=True)).cpu()
    assert int(((prod * y.double()) < 0).sum()) > shape[0] * shape[1] * shape[2] // 4        # the cancelling half is there
    if y_dtype == F32:
        u = sk.f32_ulps_from(out, ref, unit=torch.maximum(torch.maximum(prod.abs(), y.double().abs()), ref.abs()))
        print(f"[support] masked_accumulate_ mixed signs f32: {u:.3f} fp32 ulp of the larger operand from fp64")
        assert u <= 2.0
    else:
        sk.check_bf16("masked_accumulate_ mixed signs bf16", out, ref, 1e-6)


def test_masked_accumulate_past_the_grid_cap(ops, gpu):
    """The residual stream's own shape [1, 4608, 3072] (fp32 destination, accumulate, row scale): 1.7 grid-stride trips. The reference
    is fp64 on the device."""
    g = torch.Generator().manual_seed(44)
    shape, alpha = (1, 4608, 3072), 0.7
    assert shape[1] * shape[2] // 8 > GRID_CAP
    y, x = _macc_inputs(shape, g, gpu)
    rs = torch.rand(shape[1], generator=g).to(gpu)
    ref = (rs.double() * _f32(alpha))[None, :, None] * x.double() + y.double()
    out = sk.twice(lambda: ops.masked_accumulate_(y.clone(), x, rs, alpha=alpha, accumulate=True))
    u = sk.f32_ulps_from(out, ref)
    print(f"[support] masked_accumulate_ [1, 4608, 3072] f32: {u:.3f} fp32 ulp from fp64")
    assert u <= 2.0


@pytest.mark.parametrize("n", [3072, 28 * 3072 + 1])
def test_silu_split(ops, gpu, n):
    """hi = bf16(silu(x)) within one bf16 ulp of the fp64 SiLU, and hi + lo carries about 16 bits of it:
    |hi + lo - silu(x)| <= 2^-15 |silu(x)| + 1e-7 (what the skinny GEMM depends on). Without SiLU the split is bit-exact:
    hi = bf16(x), lo = bf16(x - hi). One even and one odd n."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3.0
    x[:4] = torch.tensor([0.0, -0.0, 30.0, -30.0])
    dx = x.to(gpu)
    hi, lo = (t.cpu() for t in sk.twice(lambda: ops.silu_split(dx, apply_silu=True)))
    ref = x.double() * torch.sigmoid(x.double())
    d = sk.ulp_distance(hi, ref.to(BF16))
    two = (hi.double() + lo.double() - ref).abs()
    print(f"[support] silu_split n={n}: hi {d} bf16 ulp from bf16(fp64 silu); max |hi+lo-silu| / (2^-15|silu| + 1e-7) "
          f"{float((two / (ref.abs() * 2.0 ** -15 + 1e-7)).max()):.3f}")
    assert d <= 1
    assert bool((two <= ref.abs() * 2.0 ** -15 + 1e-7).all())
    hi0, lo0 = (t.cpu() for t in sk.twice(lambda: ops.silu_split(dx, apply_silu=False)))
    assert sk.same_bits(hi0, x.to(BF16))
    assert sk.same_bits(lo0, (x - x.to(BF16).float()).to(BF16))


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("B", [1, 2])
def test_add_rows(ops, gpu, B, with_b):
    """y[r] = (y[r] + a[r % B]) + b[r % B] on 28 rows of 3072 fp32: bit-exact against that association order in fp32 on the CPU."""
    rows, D = 28, 3072
    g = torch.Generator().manual_seed(50 + B + 2 * with_b)
    y = torch.randn(rows, D, generator=g)
    a = torch.randn(B, D, generator=g) * 3.0
    b = torch.randn(B, D, generator=g) * 0.1 if with_b else None
    idx = torch.arange(rows) % B
    ref = y + a[idx]
    if with_b:
        ref = ref + b[idx]
    da, db = a.to(gpu), (b.to(gpu) if with_b else None)
    out = sk.twice(lambda: ops.add_rows_(y.to(gpu), da, db)).cpu()
    assert sk.same_bits(out, ref)
    assert sk.same_bits(da.cpu(), a)
