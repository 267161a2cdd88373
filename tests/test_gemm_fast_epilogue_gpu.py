"""rt_gemm_bf16's straight-line epilogue of interior tiles (csrc/gemm_bf16.hip: epilogue_fast) against the general one (epilogue_tile),
bit for bit, and pack_bf16x2 (csrc/rt_common.h) against torch's float32 -> bfloat16 conversion.

rt_gemm_epilogue_variant(1), the default, lets a tile that lies wholly inside M x N and on one side of gelu_from take epilogue_fast
when its group writes bf16 in 16-byte steps and has no term but the bias and GELU; variant 0 sends every tile through epilogue_tile.
Every case below runs the same launch under both on identical inputs and asks for torch.equal on every output buffer, the padding
around the output included (a sentinel: nothing outside the [M, N] view may be written). The cases are the ones at which the choice
can go wrong: all tiles interior; interior and ragged tiles in one launch; two problems of different height in one launch; gelu_from
at a tile edge and 4 columns inside a tile (that tile must stay general); an output whose rows are not 16-byte addressable (general);
the non-rope tiles of a fused q/k launch. The f32 launches of the loop (gate + residual aliasing C, add2, rowscale / alpha,
rows_per_batch equal to and half of the tile height, flat and batched) take epilogue_tile under both variants — a straight-line form of
them was measured and left out (profiles/gemm_epilogue_ab.json) — and stay here so that the switch is seen to leave them alone.
K = 128 throughout: two K-tiles, both LDS buffers."""
import pytest
import torch

from support_kernels import BF16, F32, SENT, bits

pytestmark = pytest.mark.gpu

K = 128


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


@pytest.fixture(scope="module")
def lib(gpu):
    import reptext_amd.native as native

    return native.load()


class Inputs:
    """Seeded operands and terms of one [B, M, N] problem, on the device. Outputs are made afresh per run (out())."""

    def __init__(self, dev, B, M, N, seed, gate_rows=None):
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)
        self.B, self.M, self.N, self.dev = B, M, N, dev
        self.a = rn(B, M, K).to(BF16).to(dev)
        self.w = (0.1 * rn(N, K)).to(BF16).to(dev)
        self.bias = rn(N).to(BF16).to(dev)
        self.gate = (rn(gate_rows or B, N) + 1.5).to(dev)
        self.res32 = rn(B, M, N)                                   # not representable in bf16
        self.add2 = rn(B, M, N).to(BF16).to(dev)
        self.rs_rows = torch.rand(M, generator=g) + 0.25

    def out(self, dtype, pad=8, fill=SENT):
        """(buffer, [B, M, N] view): rows of N + pad elements and one row behind every batch entry, all holding `fill`."""
        buf = torch.full((self.B, self.M + 1, self.N + pad), fill, dtype=dtype, device=self.dev)
        return buf, buf[:, : self.M, : self.N]


def both(lib, run):
    """run() under variant 0 and under variant 1; every returned buffer must be the same, bit for bit."""
    prev = lib.rt_gemm_epilogue_variant(-1)
    try:
        lib.rt_gemm_epilogue_variant(0)
        assert lib.rt_gemm_epilogue_variant(-1) == 0
        general = run()
        lib.rt_gemm_epilogue_variant(1)
        assert lib.rt_gemm_epilogue_variant(-1) == 1
        fast = run()
    finally:
        lib.rt_gemm_epilogue_variant(prev)
    torch.cuda.synchronize()
    assert len(general) == len(fast)
    for i, (u, v) in enumerate(zip(general, fast)):
        assert u.shape == v.shape and u.dtype == v.dtype
        assert torch.equal(bits(u), bits(v)), f"buffer {i}: {int((bits(u) != bits(v)).sum())} of {u.numel()} elements differ"
        assert bool((u != SENT).any()), "the launch wrote nothing"
    return fast


def test_switch_queries_and_restores(lib):
    prev = lib.rt_gemm_epilogue_variant(-1)
    assert prev in (0, 1)
    assert lib.rt_gemm_epilogue_variant(0) == prev and lib.rt_gemm_epilogue_variant(-1) == 0
    assert lib.rt_gemm_epilogue_variant(1) == 0 and lib.rt_gemm_epilogue_variant(-1) == 1
    lib.rt_gemm_epilogue_variant(prev)


# ------------------------------------------------------------------------------------------------ the bf16 kind
@pytest.mark.parametrize("M,N", [(512, 512), (300, 520)], ids=["all_interior", "interior_and_edge"])
@pytest.mark.parametrize("gelu", [None, 0], ids=["plain", "gelu"])
def test_bf16_kind(ops, lib, gpu, M, N, gelu):
    d = Inputs(gpu, 1, M, N, 1)

    def run():
        buf, out = d.out(BF16)
        ops.linear(d.a, d.w, out, bias=d.bias, gelu_from=gelu)
        return [buf]

    both(lib, run)


@pytest.mark.parametrize("gelu_from", [0, 256, 260])
def test_bf16_gelu_boundary(ops, lib, gpu, gelu_from):
    """256: the boundary is a tile edge, both tile columns are uniform. 260: the second tile column holds the boundary and stays general."""
    d = Inputs(gpu, 1, 512, 512, 2)

    def run():
        buf, out = d.out(BF16)
        ops.linear(d.a, d.w, out, bias=d.bias, gelu_from=gelu_from)
        return [buf]

    buf = both(lib, run)[0]
    # the boundary is where it was asked for: the same launch without GELU agrees left of it and nowhere else on a whole column
    _, plain = d.out(BF16)
    ops.linear(d.a, d.w, plain, bias=d.bias)
    got = buf[:, :512, :512]
    assert torch.equal(bits(got[..., :gelu_from]), bits(plain[..., :gelu_from]))
    assert not bool((got[..., gelu_from:] == plain[..., gelu_from:]).all(dim=1).any())


def test_bf16_narrow_store(ops, lib, gpu):
    """ldc % 8 != 0: rows are not 16-byte addressable, the group keeps the 8-byte stores of the general path."""
    d = Inputs(gpu, 1, 512, 512, 3)

    def run():
        buf, out = d.out(BF16, pad=4)
        ops.linear(d.a, d.w, out, bias=d.bias, gelu_from=256)
        return [buf]

    both(lib, run)


def test_two_problem_group(ops, lib, gpu):
    d0, d1 = Inputs(gpu, 1, 512, 512, 4), Inputs(gpu, 1, 256, 512, 5)
    P = ops.LinearProblem

    def run():
        (b0, o0), (b1, o1) = d0.out(BF16), d1.out(BF16)
        ops.linear_grouped([P(d0.a, d0.w, o0, bias=d0.bias, gelu_from=0), P(d1.a, d1.w, o1, bias=d1.bias, gelu_from=0)])
        (c0, x0), (c1, x1) = d0.out(F32), d1.out(F32)
        x0.copy_(d0.res32)
        x1.copy_(d1.res32)
        ops.linear_grouped([P(d0.a, d0.w, x0, bias=d0.bias, gate=d0.gate, res=x0, add2=d0.add2), P(d1.a, d1.w, x1, bias=d1.bias, gate=d1.gate, res=x1)])
        return [b0, b1, c0, c1]

    both(lib, run)


# ------------------------------------------------------------------------------------------------ the f32 kind
@pytest.mark.parametrize("M,N", [(512, 512), (300, 520)], ids=["all_interior", "interior_and_edge"])
@pytest.mark.parametrize("terms", ["gate_res", "add2", "rowscale", "add2_rowscale_alpha"])
def test_f32_kind_residual_aliases_c(ops, lib, gpu, M, N, terms):
    d = Inputs(gpu, 1, M, N, 6)
    kw = {}
    if "add2" in terms:
        kw["add2"] = d.add2
    if "rowscale" in terms:
        kw["rowscale"] = d.rs_rows.to(gpu)
    if "alpha" in terms:
        kw["alpha"] = 0.75

    def run():
        buf, x = d.out(F32)
        x.copy_(d.res32)
        ops.linear(d.a, d.w, x, bias=d.bias, gate=d.gate, res=x, **kw)          # x += gate * (a w^T + bias) ...
        return [buf]

    buf = both(lib, run)[0]
    assert not torch.equal(buf[:, :M, :N].cpu(), d.res32), "the residual stream was not updated"


@pytest.mark.parametrize("rpb", [256, 128])
@pytest.mark.parametrize("batched", [False, True], ids=["flat", "batch2"])
def test_rows_per_batch(ops, lib, gpu, rpb, batched):
    """rows_per_batch = 256: every tile lies in one gate / rowscale entry (flat: the second tile row in entry 1). 128: every tile
    straddles two entries."""
    B, M = (2, 256) if batched else (1, 512)
    d = Inputs(gpu, B, M, 512, 7, gate_rows=B * (M // rpb))
    rs = d.rs_rows[:rpb].contiguous().to(gpu)

    def run():
        buf, x = d.out(F32)
        x.copy_(d.res32)
        xv = x if batched else x[0]
        ops.linear(d.a if batched else d.a[0], d.w, xv, bias=d.bias, gate=d.gate, res=xv, rowscale=rs, alpha=0.5, rows_per_batch=rpb)
        return [buf]

    both(lib, run)


def test_rope_launch_non_rope_tiles(ops, lib, gpu):
    """A fused q/k RMSNorm + RoPE launch (its own instantiation): q | k | v | mlp columns of a single block, d = 256. The q and k tiles
    take the rope epilogue under either variant; the v tile (plain) and the mlp tile (GELU) are the ones that switch."""
    dmodel, S = 256, 512
    d = Inputs(gpu, 1, S, 4 * dmodel, 8)
    g = torch.Generator().manual_seed(9)
    nq, nk = [(torch.rand(128, generator=g) + 0.5).to(BF16).to(gpu) for _ in range(2)]
    cos, sin = ops.rope_table(torch.rand(S, 3, generator=g).mul(32).floor().to(gpu))
    rope = ops.QKRope(0, dmodel, dmodel, nq, nk, cos, sin)

    def run():
        buf, out = d.out(BF16)
        ops.linear(d.a, d.w, out, bias=d.bias, gelu_from=3 * dmodel, rope=rope)
        return [buf]

    both(lib, run)


# ------------------------------------------------------------------------------------------------ pack_bf16x2
def _special_f32():
    """float32 values whose bf16 rounding exercises every rule: signed zeros, subnormals (of bf16 and below it), exact ties to even and
    to odd, one bit either side of a tie, the carry into the exponent, overflow to infinity, infinities, NaN; then random bit patterns."""
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int64).to(torch.int32)
    base = [0x00000000, 0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x007F8000, 0x007FFFFF, 0x00800000,
            0x3F800000, 0x3F808000, 0x3F808001, 0x3F807FFF, 0x3F818000, 0x3F817FFF, 0x3F818001, 0x3FFF8000, 0x3FFFFFFF,
            0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7F808000]
    spec = i32(base + [b | 0x80000000 for b in base])
    g = torch.Generator().manual_seed(10)
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (8192 - spec.numel(),), generator=g, dtype=torch.int64).to(torch.int32)
    return torch.cat([spec, rnd]).view(F32)


def test_pack_bf16x2_matches_torch(ops, gpu):
    """rt_euler_step_f32 with a zero velocity and dsigma = -1 leaves the fp32 state as it is (x + (-0) = x for every x, zeros and NaN
    included) and writes its bf16 copy through pack_bf16x2: that copy against torch's conversion of the same values. NaN compares as
    NaN (the payload and sign of a NaN are not part of the contract); everything else bit for bit."""
    x = _special_f32()
    x32 = x.clone().to(gpu)
    xb = torch.zeros(x.numel(), dtype=BF16, device=gpu)
    ops.euler_step_f32_(x32, torch.zeros(x.numel(), dtype=BF16, device=gpu), -1.0, xb)
    torch.cuda.synchronize()
    nan = torch.isnan(x)
    assert torch.equal(bits(x32.cpu())[~nan], bits(x)[~nan]) and bool(torch.isnan(x32.cpu())[nan].all()), "the step changed its state: not a pure conversion"
    want, got = x.to(BF16), xb.cpu()
    assert bool(torch.isnan(got)[nan].all()) and not bool(torch.isnan(got)[~nan].any())
    bad = bits(got)[~nan] != bits(want)[~nan]
    assert not bool(bad.any()), f"{int(bad.sum())} conversions differ, first: {x[~nan][bad][:4].view(torch.int32).tolist()}"


@pytest.mark.parametrize("variant", [0, 1])
def test_gemm_bf16_store_is_the_rounded_f32_result(ops, lib, gpu, variant):
    """The bf16 output of a launch is the RNE rounding of the f32 output of the same launch (bias and GELU only: the value before the
    store is the same in both), through the narrow, the wide and the straight-line store."""
    d = Inputs(gpu, 1, 300, 520, 11)
    prev = lib.rt_gemm_epilogue_variant(variant)
    try:
        _, o32 = d.out(F32)
        ops.linear(d.a, d.w, o32, bias=d.bias, gelu_from=256)
        for pad in (8, 4):
            _, o16 = d.out(BF16, pad=pad)
            ops.linear(d.a, d.w, o16, bias=d.bias, gelu_from=256)
            assert torch.equal(bits(o16), bits(o32.to(BF16)))
    finally:
        lib.rt_gemm_epilogue_variant(prev)
