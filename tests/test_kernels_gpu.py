"""GPU parity: each HIP kernel (through the C ABI) vs the fp32 CPU oracle on the same seeded inputs.

Tolerances are stated per test. bf16 has 8 significand bits (rel. rounding 2^-9 ≈ 2e-3); kernels accumulate
and keep statistics in fp32, so the error budget is the bf16 rounding of inputs/outputs only.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bf16r(x):
    """Round to bf16 and back: the oracle then sees exactly the values the GPU kernel reads."""
    return x.to(torch.bfloat16).to(torch.float32)


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


# ------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (512, 768, 192), (300, 260, 128), (1024, 3072, 3072), (64, 64, 4096), (768, 21504, 3072)])
def test_linear_bias(ops, gpu, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    a = bf16r(torch.randn(M, K, generator=g))
    w = bf16r(torch.randn(N, K, generator=g) * 0.05)
    b = bf16r(torch.randn(N, generator=g))
    ref = torch.nn.functional.linear(a, w, b)
    out = torch.empty(M, N, device=gpu, dtype=torch.bfloat16)
    ops.linear(a.to(gpu, torch.bfloat16), w.to(gpu, torch.bfloat16), out, bias=b.to(gpu, torch.bfloat16))
    # fp32 accumulate, one bf16 rounding of the output: rel-L2 ≤ 2^-9/sqrt(3)·~1.5
    assert rel_l2(out.float().cpu(), ref) < 3e-3
    out32 = torch.empty(M, N, device=gpu, dtype=torch.float32)
    ops.linear(a.to(gpu, torch.bfloat16), w.to(gpu, torch.bfloat16), out32, bias=b.to(gpu, torch.bfloat16))
    assert rel_l2(out32.cpu(), ref) < 2e-5      # fp32 output: accumulation-order noise only


def test_linear_identity_asymmetric(ops, gpu):
    """A = I against an asymmetric W catches a transposed C write (guide §3)."""
    n = 256
    a = torch.eye(n)
    w = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 251) / 16.0   # exact in bf16? values k/16, k<251: yes
    out = torch.empty(n, n, device=gpu, dtype=torch.float32)
    ops.linear(a.to(gpu, torch.bfloat16), w.to(gpu, torch.bfloat16), out)
    assert torch.equal(out.cpu(), w.t().contiguous())


def test_linear_full_epilogue(ops, gpu):
    """bias → GELU(cols ≥ gelu_from) → gate → alpha → rowscale → +res → +add2, batched rows (B=2)."""
    B, R, N, K = 2, 320, 512, 256
    M = B * R
    g = torch.Generator().manual_seed(7)
    a = bf16r(torch.randn(M, K, generator=g))
    w = bf16r(torch.randn(N, K, generator=g) * 0.1)
    bias = bf16r(torch.randn(N, generator=g))
    gate = torch.randn(B, N, generator=g)
    res = bf16r(torch.randn(M, N, generator=g))
    add2 = bf16r(torch.randn(M, N, generator=g))
    rowscale = torch.rand(R, generator=g)
    gelu_from, alpha = 128, 0.75
    v = torch.nn.functional.linear(a, w, bias)
    v = torch.cat([v[:, :gelu_from], orc.gelu_tanh(v[:, gelu_from:])], dim=1)
    v = v.view(B, R, N) * gate[:, None, :] * alpha * rowscale[None, :, None]
    ref = v.reshape(M, N) + res + add2
    dev = lambda t, dt=torch.bfloat16: t.to(gpu, dt)
    out = dev(res).clone()                       # res aliases out (in-place residual update)
    ops.linear(dev(a), dev(w), out, bias=dev(bias), gate=dev(gate, torch.float32), res=out, add2=dev(add2),
               rowscale=dev(rowscale, torch.float32), rows_per_batch=R, gelu_from=gelu_from, alpha=alpha)
    assert rel_l2(out.float().cpu(), ref) < 3e-3
    out32 = dev(res, torch.float32).clone()
    ops.linear(dev(a), dev(w), out32, bias=dev(bias), gate=dev(gate, torch.float32), res=out32, add2=dev(add2),
               rowscale=dev(rowscale, torch.float32), rows_per_batch=R, gelu_from=gelu_from, alpha=alpha)
    assert rel_l2(out32.cpu(), ref) < 2e-5


def test_linear_grouped_strided(ops, gpu):
    """Two problems in one launch writing row ranges of one [B*S, 3d]-like buffer (text rows first), strided A."""
    T, Nimg, d, K = 128, 384, 256, 192
    S = T + Nimg
    g = torch.Generator().manual_seed(11)
    x = bf16r(torch.randn(S, K + 64, generator=g))          # lda > K
    w_t = bf16r(torch.randn(3 * d, K, generator=g) * 0.1)
    w_i = bf16r(torch.randn(3 * d, K, generator=g) * 0.1)
    b_t = bf16r(torch.randn(3 * d, generator=g))
    b_i = bf16r(torch.randn(3 * d, generator=g))
    xd = x.to(gpu, torch.bfloat16)
    out = torch.zeros(S, 3 * d + 128, device=gpu, dtype=torch.bfloat16)    # ldc > N
    ops.linear_grouped([
        ops.LinearProblem(xd[T:, :K], w_i.to(gpu, torch.bfloat16), out[T:, : 3 * d], bias=b_i.to(gpu, torch.bfloat16)),
        ops.LinearProblem(xd[:T, :K], w_t.to(gpu, torch.bfloat16), out[:T, : 3 * d], bias=b_t.to(gpu, torch.bfloat16)),
    ])
    ref = torch.cat([torch.nn.functional.linear(x[:T, :K], w_t, b_t), torch.nn.functional.linear(x[T:, :K], w_i, b_i)])
    assert rel_l2(out[:, : 3 * d].float().cpu(), ref) < 3e-3
    assert float(out[:, 3 * d :].float().abs().max()) == 0.0   # padding columns untouched


def test_linear_model_shapes(ops, gpu):
    """rt_gemm_bf16 at the model's launch shapes — the full epilogue, grouped problems, bf16 and fp32 outputs, several rounds of
    tiles and a ragged last row/column of tiles: finite, bitwise repeatable, and against an fp32 reference."""
    g = torch.Generator(device=gpu).manual_seed(3)
    rn = lambda *s, sc=1.0: (torch.randn(*s, device=gpu, generator=g) * sc).to(torch.bfloat16)
    cases = []
    # (a) 4608 x 3072, fp32 out + gate + residual (single-block out-projection)
    a, w, b = rn(4608, 1024), rn(3072, 1024, sc=0.05), rn(3072)
    gate, res = torch.randn(1, 3072, device=gpu, generator=g), torch.randn(4608, 3072, device=gpu, generator=g)
    cases.append(("4608x3072 f32", lambda out: ops.linear(a, w, out, bias=b, gate=gate, res=res), torch.float32, (4608, 3072)))
    cases.append(("4608x3072 bf16 gelu", lambda out: ops.linear(a, w, out, bias=b, gelu_from=1024), torch.bfloat16, (4608, 3072)))
    # (b) grouped image + text rows, N = 12288 (ff1: 864 tiles) and N = 9216 (qkv: 648 tiles)
    x = rn(4608, 512)
    for N in (12288, 9216):
        wi, wt, bi, bt = rn(N, 512, sc=0.05), rn(N, 512, sc=0.05), rn(N), rn(N)
        cases.append((f"grouped N={N}", (lambda out, wi=wi, wt=wt, bi=bi, bt=bt: ops.linear_grouped(
            [ops.LinearProblem(x[512:], wi, out[512:], bias=bi, gelu_from=0), ops.LinearProblem(x[:512], wt, out[:512], bias=bt, gelu_from=0)])),
            torch.bfloat16, (4608, N)))
    # (c) one problem, ragged rows, several rounds
    a2, w2 = rn(4000, 256), rn(5120, 256, sc=0.05)
    cases.append(("ragged M=4000 N=5120", lambda out: ops.linear(a2, w2, out), torch.float32, (4000, 5120)))
    first = {}
    for name, run, dt, shape in cases:
        outs = []
        for _ in range(2):
            out = torch.full(shape, float("nan"), device=gpu, dtype=dt)
            run(out)
            outs.append(out)
        assert bool(torch.isfinite(outs[0].float()).all()), name
        assert torch.equal(outs[1], outs[0]), name
        first[name] = outs[0]
    assert rel_l2(first["ragged M=4000 N=5120"], torch.nn.functional.linear(a2.float(), w2.float())) < 2e-5
    o = torch.empty(4608, 3072, device=gpu, dtype=torch.float32)
    ops.linear(a, w, o)
    assert rel_l2(o, torch.nn.functional.linear(a.float(), w.float())) < 2e-5


def test_linear_rejects_bad_args(ops, gpu):
    from reptext_amd.native import NativeCallError

    a = torch.zeros(64, 96, device=gpu, dtype=torch.bfloat16)      # K=96 not a multiple of 64
    w = torch.zeros(64, 96, device=gpu, dtype=torch.bfloat16)
    out = torch.zeros(64, 64, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(NativeCallError):
        ops.linear(a, w, out)
    with pytest.raises(RuntimeError):
        ops.linear(a.cpu(), w, out)                                  # CPU tensor: error, never a fallback


# ------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("D,xdtype", [(3072, torch.bfloat16), (3072, torch.float32), (512, torch.bfloat16), (4096, torch.bfloat16), (64, torch.float32)])
def test_layernorm_modulate(ops, gpu, D, xdtype):
    B, R = 2, 37
    g = torch.Generator().manual_seed(D)
    x = torch.randn(B, R, D, generator=g) * 3 + 0.5
    if xdtype == torch.bfloat16:
        x = bf16r(x)
    shift, scale = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    ref = orc.layer_norm(x) * (1 + scale[:, None]) + shift[:, None]
    mod = torch.cat([shift, scale], dim=1).to(gpu)                 # one [B, 2D] buffer, chunk views
    out = torch.empty(B, R, D, device=gpu, dtype=torch.bfloat16)
    ops.layernorm_modulate(x.to(gpu, xdtype), out, mod[:, :D], mod[:, D:])
    assert rel_l2(out.float().cpu(), ref) < 3e-3
    out2 = torch.empty(B, R, D, device=gpu, dtype=torch.bfloat16)
    ops.layernorm_modulate(x.to(gpu, xdtype), out2, None, None)
    assert rel_l2(out2.float().cpu(), orc.layer_norm(x)) < 3e-3


def test_qk_rmsnorm_rope(ops, gpu):
    B, T, Nimg, H = 2, 24, 40, 3
    S, d = T + Nimg, H * 128
    g = torch.Generator().manual_seed(5)
    buf = bf16r(torch.randn(B, S, 3 * d, generator=g))
    ws = [bf16r(1 + 0.1 * torch.randn(128, generator=g)) for _ in range(4)]   # q_txt, k_txt, q_img, k_img
    ids = torch.cat([torch.zeros(T, 3), orc.latent_image_ids(10, 16)], dim=0)
    cos, sin = orc.rope_table(ids)
    q, k = buf[..., :d].reshape(B, S, H, 128), buf[..., d : 2 * d].reshape(B, S, H, 128)
    qn = torch.cat([orc.rms_norm(q[:, :T], ws[0]), orc.rms_norm(q[:, T:], ws[2])], dim=1)
    kn = torch.cat([orc.rms_norm(k[:, :T], ws[1]), orc.rms_norm(k[:, T:], ws[3])], dim=1)
    ref = buf.clone()
    ref[..., :d] = orc.apply_rope(qn, cos, sin).reshape(B, S, d)
    ref[..., d : 2 * d] = orc.apply_rope(kn, cos, sin).reshape(B, S, d)
    dbuf = buf.to(gpu, torch.bfloat16)
    wd = [w.to(gpu, torch.bfloat16) for w in ws]
    ops.qk_rmsnorm_rope(dbuf, 0, d, H, T, wd[0], wd[1], wd[2], wd[3], cos.to(gpu), sin.to(gpu))
    assert rel_l2(dbuf[..., : 2 * d].float().cpu(), ref[..., : 2 * d]) < 3e-3
    assert torch.equal(dbuf[..., 2 * d :].float().cpu(), buf[..., 2 * d :])     # v untouched


def test_rope_and_timestep_tables(ops, gpu):
    ids = torch.cat([torch.zeros(16, 3), orc.latent_image_ids(128, 128)], dim=0)
    cos, sin = ops.rope_table(ids.to(gpu))
    rc, rs = orc.rope_table(ids)
    assert float((cos.cpu() - rc).abs().max()) < 2e-6 and float((sin.cpu() - rs).abs().max()) < 2e-6
    t = torch.tensor([1000.0, 622.459, 3500.0, 0.0])
    emb = ops.timestep_embedding(t.to(gpu))
    # fp32 sin/cos of arguments up to 3.5e3: device vs host libm differ by a few ulp of the ARGUMENT (~2e-4 abs)
    assert float((emb.cpu() - orc.timestep_embedding(t)).abs().max()) < 5e-4


def test_gemv(ops, gpu):
    B, N, K = 3, 1000, 3072
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, K, generator=g)
    w = bf16r(torch.randn(N, K, generator=g) * 0.02)
    b = bf16r(torch.randn(N, generator=g))
    y = torch.empty(B, N, device=gpu)
    ops.gemv(x.to(gpu), w.to(gpu, torch.bfloat16), b.to(gpu, torch.bfloat16), y, silu_in=True)
    ref = torch.nn.functional.linear(orc.silu(x), w, b)
    assert rel_l2(y.cpu(), ref) < 1e-5
    ops.gemv(x.to(gpu), w.to(gpu, torch.bfloat16), None, y, silu_out=True, accumulate=True)
    ref2 = ref + orc.silu(torch.nn.functional.linear(x, w))
    assert rel_l2(y.cpu(), ref2) < 1e-5


# ------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("B,S,H", [(1, 128, 1), (2, 768, 3), (1, 200, 2), (1, 4608, 2)])
def test_attention(ops, gpu, B, S, H):
    d = H * 128
    g = torch.Generator().manual_seed(S)
    qkv = bf16r(torch.randn(B, S, 3 * d, generator=g))
    qkv[..., :d] *= 2.0                      # sharper softmax than N(0,1) scores
    q, k, v = (qkv[..., i * d : (i + 1) * d].reshape(B, S, H, 128) for i in range(3))
    ref = orc.attention(q, k, v)
    dq = qkv.to(gpu, torch.bfloat16)
    out = torch.empty(B, S, d, device=gpu, dtype=torch.bfloat16)
    ops.attention(dq[..., :d], dq[..., d : 2 * d], dq[..., 2 * d :], out, H)
    # P is rounded to bf16 before P·V and the output once more: ≈ 2·2^-9/sqrt(3)
    assert rel_l2(out.float().cpu(), ref) < 5e-3
    # in place over q
    ops.attention(dq[..., :d], dq[..., d : 2 * d], dq[..., 2 * d :], dq[..., :d], H)
    assert torch.equal(dq[..., :d], out)


def test_attention_online_softmax_rescale(ops, gpu):
    """Force the running-max rescale: one late key dominates one query row (guide §5.4 rule 26)."""
    B, S, H = 1, 512, 1
    g = torch.Generator().manual_seed(1)
    q = bf16r(torch.randn(B, S, H, 128, generator=g))
    k = bf16r(torch.randn(B, S, H, 128, generator=g))
    v = bf16r(torch.randn(B, S, H, 128, generator=g))
    k[0, 300, 0] = q[0, 17, 0] * 4.0          # score jumps by ~4·|q|²/sqrt(128) ≈ 45 at key tile 4
    k[0, 450, 0] = q[0, 100, 0] * 6.0
    k = bf16r(k)
    ref = orc.attention(q, k, v)
    dq, dk, dv = (t.reshape(B, S, 128).to(gpu, torch.bfloat16) for t in (q, k, v))
    buf = torch.cat([dq, dk, dv], dim=-1).contiguous()
    out = torch.empty(B, S, 128, device=gpu, dtype=torch.bfloat16)
    ops.attention(buf[..., :128], buf[..., 128:256], buf[..., 256:], out, H)
    assert rel_l2(out.float().cpu(), ref) < 5e-3
    assert float((out.float().cpu()[0, 17] - ref[0, 17]).abs().max()) < 0.05


@pytest.mark.parametrize("B,S,H", [(1, 256, 2), (2, 768, 3), (1, 1024, 24), (1, 4608, 4)])
def test_attention_v3_variant(ops, gpu, B, S, H):
    """csrc/attention_v3.hip (one wave per SIMD, 64 query rows per wave, O and Q in asm-owned accumulator registers, speculative
    numerators with a deferred decision) on the shapes it takes (S % 256 == 0): against the fp32 oracle, against attention.hip on
    the same buffers, with a key that spikes LATE for one query row in each 32-row block position (the rescale path must fire
    in both query blocks of a wave; the three keys sit at positions 58, 44 and 33 of their tiles, so all in the SECOND 32-key half:
    every position of a tile, both halves, is tests/test_attention_v3_edges_gpu.py's), bitwise repeatable, in place over q."""
    from reptext_amd import native

    lib = native.load()
    d = H * 128
    g = torch.Generator().manual_seed(S + H)
    qkv = bf16r(torch.randn(B, S, 3 * d, generator=g))
    qkv[..., :d] *= 2.0
    q, k, v = (qkv[..., i * d : (i + 1) * d].reshape(B, S, H, 128) for i in range(3))
    # spikes: query rows 5 (block a of wave 0) and 40 (block b), 200 (wave 3): keys late in the sequence, all in the second half of their tile
    for qrow, krow in ((5, S - 70), (40, S - 20), (200, S // 2 + 33)):
        k[0, krow, 0] = q[0, qrow, 0] * 3.0
    qkv = torch.cat([q.reshape(B, S, d), k.reshape(B, S, d), v.reshape(B, S, d)], dim=-1)
    ref = orc.attention(q, k, v)
    dq = qkv.to(gpu, torch.bfloat16)
    prev = lib.rt_attention_variant(-1)
    try:
        lib.rt_attention_variant(2)
        out3 = torch.empty(B, S, d, device=gpu, dtype=torch.bfloat16)
        ops.attention(dq[..., :d], dq[..., d : 2 * d], dq[..., 2 * d :], out3, H)
        again = torch.empty_like(out3)
        ops.attention(dq[..., :d], dq[..., d : 2 * d], dq[..., 2 * d :], again, H)
        lib.rt_attention_variant(0)
        out1 = torch.empty_like(out3)
        ops.attention(dq[..., :d], dq[..., d : 2 * d], dq[..., 2 * d :], out1, H)
        e3, e1, e31 = rel_l2(out3.float().cpu(), ref), rel_l2(out1.float().cpu(), ref), rel_l2(out3.float(), out1.float())
        print(f"attention v3 B={B} S={S} H={H}: {e3:.3e} vs fp32 oracle (attention.hip {e1:.3e}); v3 vs attention.hip {e31:.3e}")
        assert bool(torch.isfinite(out3.float()).all()) and e3 < 5e-3 and torch.equal(out3, again)
        for qrow in (5, 40, 200):
            assert float((out3.float().cpu()[0, qrow, :128] - ref.reshape(B, S, d)[0, qrow, :128]).abs().max()) < 0.08, qrow
        lib.rt_attention_variant(2)
        inplace = dq.clone()
        ops.attention(inplace[..., :d], inplace[..., d : 2 * d], inplace[..., 2 * d :], inplace[..., :d], H)
        assert torch.equal(inplace[..., :d], out3)
    finally:
        lib.rt_attention_variant(prev)


# ------------------------------------------------------------------------------------------- elementwise
def test_euler_pack_cast_mask(ops, gpu):
    g = torch.Generator().manual_seed(2)
    x = bf16r(torch.randn(2, 4096, 64, generator=g))
    v = bf16r(torch.randn(2, 4096, 64, generator=g))
    dx = x.to(gpu, torch.bfloat16)
    ops.euler_step_(dx, v.to(gpu, torch.bfloat16), -0.0116)
    ref = orc.euler_step(x.to(torch.bfloat16), v.to(torch.bfloat16), 1.0, 1.0 - 0.0116)
    assert torch.equal(dx.cpu(), ref)         # fp32 axpy + one rounding: bit-exact

    lat = bf16r(torch.randn(2, 16, 32, 48, generator=g))
    packed = ops.pack_latents(lat.to(gpu, torch.bfloat16))
    assert torch.equal(packed.float().cpu(), orc.pack_latents(lat))
    nhwc = ops.unpack_latents_nhwc(packed, 32, 48, 0.3611, 0.1159)
    ref_u = bf16r(orc.unpack_latents(orc.pack_latents(lat), 16 * 16, 24 * 16) / 0.3611 + 0.1159)
    assert float((nhwc.float().cpu().permute(0, 3, 1, 2) - ref_u).abs().max()) <= 2 ** -6   # 1 bf16 ulp at |x|<4 (mul vs div)

    f = torch.randn(1000, generator=g)
    assert torch.equal(ops.to_bf16(f.to(gpu)).cpu(), f.to(torch.bfloat16))
    assert torch.equal(ops.to_f32(f.to(gpu, torch.bfloat16)).cpu(), f.to(torch.bfloat16).float())

    y = bf16r(torch.randn(2, 96, 256, generator=g))
    xx = bf16r(torch.randn(2, 96, 256, generator=g))
    mask = torch.rand(96, generator=g)
    dy = y.to(gpu, torch.bfloat16)
    ops.masked_accumulate_(dy, xx.to(gpu, torch.bfloat16), mask.to(gpu), alpha=0.5)
    assert rel_l2(dy.float().cpu(), y + 0.5 * mask[None, :, None] * xx) < 3e-3
    u = ops.cfg_mix(y.to(gpu, torch.bfloat16), xx.to(gpu, torch.bfloat16), 3.5)
    assert rel_l2(u.float().cpu(), y + 3.5 * (xx - y)) < 3e-3


# ------------------------------------------------------------------------------------------------ fp8 (BASELINE config 5)
FP8 = torch.float8_e4m3fn


def _quant_rows_ref(x):
    """The kernel's arithmetic on the CPU: scale = amax/448 (fp32), q = e4m3(clamp(x * (1/scale)))."""
    x = x.float()
    amax = x.abs().amax(dim=1)
    sc = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    y = (x * (1.0 / sc)[:, None]).clamp(-448.0, 448.0)
    return y.to(FP8), sc


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantize_rows_fp8(ops, gpu, dtype):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(37, 3072, generator=g) * torch.logspace(-3, 2, 37)[:, None]).to(dtype)
    x[5] = 0                                                          # all-zero row -> scale 1, zeros
    q, sc = ops.quantize_rows_fp8(x.to(gpu))
    qr, scr = _quant_rows_ref(x)
    assert torch.equal(sc.cpu(), scr)
    a, b = q.cpu().view(torch.uint8), qr.view(torch.uint8)
    mism = (a != b)
    # identical arithmetic on both sides; tolerate the odd last-place tie between the device reciprocal and the host's
    assert mism.float().mean() < 1e-3, float(mism.float().mean())
    assert rel_l2(q.cpu().float() * sc.cpu()[:, None], x.float()) < 4e-2      # e4m3: 3 mantissa bits
    assert float(q.cpu().float().abs().max()) <= 448.0


@pytest.mark.parametrize("M,N,K,batch", [(256, 256, 128, 1), (300, 520, 384, 1), (512, 768, 3072, 2)])
def test_gemm_fp8_exact_operands(ops, gpu, M, N, K, batch):
    """e4m3 x e4m3 products are exact in fp32, so with f32 output the kernel must match an fp32 matmul of the de-quantised
    operands to accumulation-order noise: this pins the operand layout of v_mfma_scale_f32_16x16x128_f8f6f4 (each lane
    group's 32 k-values are taken as chunks j and j+4 of the 128-byte tile row, for both operands)."""
    g = torch.Generator().manual_seed(M + N + K)
    a8 = torch.randn(batch, M, K, generator=g).to(FP8)
    w8 = (torch.randn(N, K, generator=g) * 0.5).to(FP8)
    sa = torch.rand(batch * M, generator=g) + 0.5
    sw = torch.rand(N, generator=g) * 0.02 + 0.01
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
    ref = torch.einsum("bmk,nk->bmn", a8.float().double(), w8.float().double()) * sa.view(batch, M, 1).double() * sw.view(1, 1, N).double() + bias.double()
    out = torch.empty(batch, M, N, device=gpu, dtype=torch.float32)
    ops.linear(a8.to(gpu), w8.to(gpu), out, bias=bias.to(gpu), a_scale=sa.to(gpu), w_scale=sw.to(gpu))
    err = rel_l2(out.cpu(), ref)
    print(f"gemm fp8 {M}x{N}x{K} b{batch} f32-out rel-L2 {err:.2e}")
    assert err < 2e-5
    # bf16 output + GELU on the upper columns + grouped launch with a second problem (image + text stream shape)
    out16 = torch.empty(batch, M, N, device=gpu, dtype=torch.bfloat16)
    a2 = torch.randn(1, 64, K, generator=g).to(FP8)
    out2 = torch.empty(1, 64, N, device=gpu, dtype=torch.bfloat16)
    ops.linear_grouped([ops.LinearProblem(a8.to(gpu), w8.to(gpu), out16, bias=bias.to(gpu), a_scale=sa.to(gpu), w_scale=sw.to(gpu), gelu_from=N // 2),
                        ops.LinearProblem(a2.to(gpu), w8.to(gpu), out2, w_scale=sw.to(gpu))])
    refg = ref.clone()
    refg[..., N // 2:] = orc.gelu_tanh(ref[..., N // 2:].float()).double()
    assert rel_l2(out16.float().cpu(), refg) < 3e-3
    ref2 = torch.einsum("bmk,nk->bmn", a2.float().double(), w8.float().double()) * sw.view(1, 1, N).double()
    assert rel_l2(out2.float().cpu(), ref2) < 3e-3


def test_gemm_fp8_rejects_bad_shapes(ops, gpu):
    from reptext_amd import native

    a = torch.zeros(64, 192, device=gpu, dtype=FP8)           # K % 128 != 0
    w = torch.zeros(64, 192, device=gpu, dtype=FP8)
    with pytest.raises(native.NativeCallError):
        ops.linear(a, w, torch.empty(64, 64, device=gpu, dtype=torch.bfloat16))
    with pytest.raises(TypeError):                             # mixed operand dtypes
        ops.linear(torch.zeros(64, 256, device=gpu, dtype=FP8), torch.zeros(64, 256, device=gpu, dtype=torch.bfloat16),
                   torch.empty(64, 64, device=gpu, dtype=torch.bfloat16))


@pytest.mark.parametrize("xdtype", [torch.bfloat16, torch.float32])
def test_layernorm_modulate_fp8(ops, gpu, xdtype):
    g = torch.Generator().manual_seed(9)
    B, R, D = 2, 70, 3072
    x = (torch.randn(B, R, D, generator=g) * 3 + 0.5).to(xdtype)
    shift, scale = torch.randn(B, D, generator=g) * 0.3, torch.randn(B, D, generator=g) * 0.3
    y = orc.layer_norm(x.float()) * (1 + scale[:, None]) + shift[:, None]
    qr, scr = _quant_rows_ref(y.reshape(B * R, D))
    out = torch.empty(B, R, D, device=gpu, dtype=FP8)
    rs = torch.empty(B * R, device=gpu, dtype=torch.float32)
    ops.layernorm_modulate_fp8(x.to(gpu), out, rs, shift.to(gpu), scale.to(gpu))
    assert rel_l2(rs.cpu(), scr) < 1e-5
    deq = out.cpu().float().reshape(B * R, D) * rs.cpu()[:, None]
    assert rel_l2(deq, y.reshape(B * R, D)) < 4e-2                      # e4m3 rounding floor (2^-4 relative, uniform: ~2.6e-2)
    mism = (out.cpu().view(torch.uint8).reshape(B * R, D) != qr.view(torch.uint8)).float().mean()
    assert mism < 2e-2, float(mism)                                     # fp32 LN statistics differ in the last place -> a few ties flip


@pytest.mark.parametrize("B,S,H,T", [(1, 256, 2, 64), (2, 200, 3, 40), (1, 1100, 2, 0)])
def test_attention_fp8(ops, gpu, B, S, H, T):
    """rt_attention_fp8_prep + rt_attention_fp8_fwd vs the oracle's attention with the same static e4m3 quantisation (tight:
    operand layout, key permutation of Vᵀ, masking of ragged tiles) and vs the fp32 attention (the e4m3 floor)."""
    g = torch.Generator().manual_seed(S + H)
    d = H * 128
    qkv = bf16r(torch.randn(B, S, 3 * d, generator=g))
    w = [bf16r(1.0 + 0.1 * torch.randn(128, generator=g)) for _ in range(4)]        # q_txt, k_txt, q_img, k_img
    ids = torch.cat([torch.zeros(T, 3), orc.latent_image_ids(2 * 10, 2 * ((S - T + 9) // 10))[: S - T]]) if S - T > 0 else torch.zeros(T, 3)
    cos, sin = orc.rope_table(ids)
    heads = lambda x: x.reshape(B, S, H, 128)
    q, k, v = heads(qkv[..., :d]), heads(qkv[..., d:2 * d]), heads(qkv[..., 2 * d:])

    def norm(x, wt, wi):
        y = torch.empty_like(x)
        y[:, :T] = orc.rms_norm(x[:, :T], wt)
        y[:, T:] = orc.rms_norm(x[:, T:], wi)
        return orc.apply_rope(y, cos, sin)

    qn, kn = norm(q, w[0], w[2]), norm(k, w[1], w[3])
    ref = orc.attention(qn, kn, v)
    with orc.fp8_attention():
        ref8 = orc.attention(qn, kn, v)
    dev = lambda t: t.to(gpu, torch.bfloat16)
    qk8 = torch.empty(B, S, 2 * d, device=gpu, dtype=FP8)
    from reptext_amd import native
    vt8 = torch.empty(int(native.load().rt_attention_fp8_vt_bytes(B, S, H)), device=gpu, dtype=FP8)
    buf = dev(qkv)
    keep = buf.clone()
    ops.attention_fp8_prep(buf, 0, d, 2 * d, H, T, dev(w[0]), dev(w[1]), dev(w[2]), dev(w[3]), cos.to(gpu), sin.to(gpu), qk8, vt8)
    assert torch.equal(buf, keep)                                     # prep does not modify the projection buffer
    # the prep output itself: q|k = e4m3(16 · RoPE(RMSNorm(.)))
    qk_ref = torch.cat([qn.reshape(B, S, d), kn.reshape(B, S, d)], dim=-1)
    assert rel_l2(qk8.float().cpu() / 16.0, qk_ref) < 4e-2
    out = torch.empty(B, S, d, device=gpu, dtype=torch.bfloat16)
    ops.attention_fp8(qk8, vt8, out, H)
    e8, e32 = rel_l2(out.float().cpu(), ref8), rel_l2(out.float().cpu(), ref)
    floor = rel_l2(ref8, ref)
    print(f"attention fp8 B={B} S={S} H={H}: {e8:.3e} vs e4m3 oracle, {e32:.3e} vs fp32 oracle (floor {floor:.3e})")
    # The numerators are e4m3 (3 mantissa bits) and their rounding grid follows the kernel's running max, which the oracle's
    # true row max does not reproduce: on random v the two e4m3 runs are independent draws around the fp32 result.
    assert e32 < 1.25 * floor + 2e-3 and e8 < 1.45 * floor + 2e-3
    # discriminating checks that do not depend on the numerator grid:
    # (1) q = 0 -> uniform attention -> every row is the mean of the e4m3 values of v
    qk0 = qk8.clone()
    qk0[..., :d] = 0
    ops.attention_fp8(qk0, vt8, out, H)
    v8 = heads(qkv[..., 2 * d:]).to(FP8).float()
    assert rel_l2(out.float().cpu(), v8.mean(dim=1, keepdim=True).expand(-1, S, -1, -1).reshape(B, S, d)) < 3e-3
    # (2) exact-arithmetic patterns: q = e_0, k_j = -pattern(j) · e_0 and scale = ln 2 make every numerator an exact power of two
    #     (e4m3-exact, no rounding anywhere but the bf16 store), so the output is sum_j 2^-pattern(j) v8_j / sum_j 2^-pattern(j).
    #     The three patterns depend on different bits of the key index and together pin the key order of Vᵀ (position inside a
    #     32-key half, half / group, tile) — a wrong permutation or operand layout is an O(1) error here.
    j = torch.arange(S)
    for name, pat in (("low bits", j % 8), ("group / half", (j >> 3) % 8), ("tile", (j >> 6) % 8)):
        qk = torch.zeros(B, S, 2 * d)
        for hd in range(H):
            qk[:, :, hd * 128] = 16.0                                  # q = e_0 (x16 prescale)
            qk[:, :, d + hd * 128] = -16.0 * pat.float()               # k_j = -pattern(j) e_0
        ops.attention_fp8(qk.to(gpu).to(FP8), vt8, out, H, scale=math.log(2.0))
        wgt = torch.exp2(-pat.double())
        exact = (wgt[None, :, None, None] * v8.double()).sum(dim=1, keepdim=True) / wgt.sum()
        err = rel_l2(out.float().cpu(), exact.expand(-1, S, -1, -1).reshape(B, S, d))
        print(f"   exact pattern '{name}': {err:.2e}")
        assert err < 3e-3, name


def test_c_abi_from_plain_cpp_host(gpu, tmp_path):
    """The boundary without Python or torch: tools/capi_smoke/capi_smoke.cpp links the shared library through the public header,
    allocates with hipMalloc and checks rt_gemm_bf16 / rt_attention_fwd against scalar CPU arithmetic."""
    import os
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "arabic-text-image-generation-reptext_amd")
    exe = str(tmp_path / "capi_smoke")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I" + os.path.join(root, "include"), os.path.join(root, "tools", "capi_smoke", "capi_smoke.cpp"),
                    "-L" + pkg, "-lrt_reptext_hip", "-Wl,-rpath," + pkg, "-o", exe], check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------- hint-side resizes
def test_resize2d_is_bit_identical_to_interpolate(ops, gpu):
    """ops.resize2d against torch.nn.functional.interpolate on the CPU: the /16 bilinear regional mask of PIPE:1010-1012
    (uint8 / 255 first), size-driven bilinear (the glyph mask, PIPE:649) and nearest (INP:813). Bit for bit wherever the
    resize ratio is a power of two (16 and 8 are what the pipelines use; all tap weights are then exact) and for nearest;
    within one fp32 ulp for other ratios, where ATen's own CPU result depends on its vector code path."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(0)
    for H, W in [(1024, 1024), (256, 384), (250, 330), (33, 17)]:
        m = (torch.rand(H, W, generator=g) > 0.6).to(torch.uint8) * 255
        m[H // 3 : H // 2, W // 4 : W // 2] = 255
        m[0, 0] = 77                                                      # a non-binary value: the division must match too
        ref = F.interpolate((m / 255.0)[None, None].float(), scale_factor=1 / 16, mode="bilinear")
        got = ops.resize2d(m.to(gpu)[None, None], scale_factor=1 / 16, mode="bilinear", u8_scale=255.0)
        assert got.shape == ref.shape and torch.equal(got.cpu(), ref), (H, W)
    x = torch.randn(2, 3, 96, 160, generator=g)
    for size in [(12, 20), (48, 80), (6, 10), (37, 51), (200, 300)]:
        for mode in ("bilinear", "nearest"):
            kw = dict(align_corners=False) if mode == "bilinear" else {}
            ref = F.interpolate(x, size=size, mode=mode, **kw)
            got = ops.resize2d(x.to(gpu), size=size, mode=mode).cpu()
            if mode == "nearest" or size in [(12, 20), (48, 80), (6, 10)]:
                assert torch.equal(got, ref), (size, mode)
            else:
                assert float((got - ref).abs().max()) <= 4.8e-7, (size, mode)      # one ulp at |x| < 4
    ref = F.interpolate(x, scale_factor=0.5, mode="bilinear")
    assert torch.equal(ops.resize2d(x.to(gpu), scale_factor=0.5, mode="bilinear").cpu(), ref)


def test_glyph_blend_matches_torch(ops, gpu):
    """PIPE:645-654: where(interpolate((img > 0).any(1)) > 0, 0.10 * lat + noise, noise) as one kernel."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(1)
    img = -torch.ones(2, 3, 256, 320)
    img[0, :, 60:120, 100:200] = torch.rand(3, 60, 100, generator=g) * 2 - 1
    img[1, 1, 7, 9] = 0.5                                                 # a single lit pixel in one channel
    lat, noise = torch.randn(2, 16, 32, 40, generator=g), torch.randn(2, 16, 32, 40, generator=g)
    m = F.interpolate((img > 0).any(dim=1, keepdim=True).float(), size=(32, 40), mode="bilinear", align_corners=False) > 0
    ref = torch.where(m, 0.10 * lat + noise, noise)
    got = ops.glyph_blend(img.to(gpu), lat.to(gpu), noise.to(gpu)).cpu()
    assert torch.equal(got, ref) and bool(m.any()) and not bool(m.all())


def test_torch_library_custom_ops_match_direct_calls(ops, gpu):
    """SURVEY §8b / north_star wording: the kernels are also registered as PyTorch custom ops (torch.ops.reptext_amd.*,
    reptext_amd/torch_ops.py). Same kernels behind the dispatcher: results are bit-identical to the direct ctypes calls, a CPU
    tensor is refused, and a whole model forward routed through the dispatcher equals the direct one."""
    import reptext_amd.torch_ops as tops
    from reptext_amd.transformer import FluxTransformer2DModel

    g = torch.Generator(device=gpu).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=gpu, generator=g).to(torch.bfloat16)
    a, w, b = r(300, 256), r(520, 256) * 0.05, r(520)
    res = torch.randn(300, 520, device=gpu, generator=g)
    o1, o2 = torch.empty(300, 520, device=gpu), torch.empty(300, 520, device=gpu)
    ops.linear(a, w, o1, bias=b, res=res, gelu_from=256)
    torch.ops.reptext_amd.linear(a, w, o2, b, None, res, None, None, 256, 1.0)
    assert torch.equal(o1, o2)
    qkv = r(2, 200, 3 * 256)
    a1, a2 = torch.empty(2, 200, 256, device=gpu, dtype=torch.bfloat16), torch.empty(2, 200, 256, device=gpu, dtype=torch.bfloat16)
    ops.attention(qkv[..., :256], qkv[..., 256:512], qkv[..., 512:], a1, 2)
    torch.ops.reptext_amd.attention(qkv[..., :256], qkv[..., 256:512], qkv[..., 512:], a2, 2)
    assert torch.equal(a1, a2)
    with pytest.raises(NotImplementedError):
        torch.ops.reptext_amd.attention(qkv.cpu()[..., :256], qkv.cpu()[..., 256:512], qkv.cpu()[..., 512:], a2.cpu(), 2)
    cfg = dict(patch_size=1, in_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=2,
               joint_attention_dim=128, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
    tr = FluxTransformer2DModel(**cfg, device=gpu, dtype=torch.bfloat16).random_init_(1)
    kw = dict(hidden_states=r(1, 64, 64), encoder_hidden_states=r(1, 32, 128), pooled_projections=r(1, 64), timestep=torch.full((1,), 0.5, device=gpu),
              guidance=torch.full((1,), 3.5, device=gpu), img_ids=orc.latent_image_ids(16, 16).to(gpu, torch.bfloat16),
              txt_ids=torch.zeros(32, 3, device=gpu, dtype=torch.bfloat16), return_dict=False)
    v_direct = tr(**kw)[0].clone()
    tops.enable_dispatch(True)
    try:
        v_dispatch = tr(**kw)[0].clone()
    finally:
        tops.enable_dispatch(False)
    assert torch.equal(v_direct, v_dispatch)
