"""GPU checks of the loop's small passes: each new form against the launches it replaces, bit for bit (torch.equal) — the skinny
adaLN GEMM vs the linear(hi) ; linear(lo, res=) pair, the two-segment LayerNorm vs two launches, time_text_embed for all steps vs
step by step, and the ModulationTable built from them."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


def _split(ops, gpu, M, K, seed):
    g = torch.Generator().manual_seed(seed)
    temb = (torch.randn(M, K, generator=g) * 2.0).to(gpu)
    return ops.silu_split(temb, apply_silu=True)


def _pair(ops, hi, lo, w, b, out):
    ops.linear(hi, w, out, bias=b)
    ops.linear(lo, w, out, res=out)


@pytest.mark.parametrize("M,N,K", [(28, 9216, 3072), (1, 9216, 3072), (8, 9216, 3072), (16, 6144, 3072), (17, 1024, 512), (32, 9216, 3072)])
def test_skinny_gemm_equals_the_two_launches(ops, gpu, M, N, K):
    hi, lo = _split(ops, gpu, M, K, 7 * M + N)
    g = torch.Generator().manual_seed(N + K + M)
    w = (torch.randn(N, K, generator=g) * 0.05).to(gpu, BF16)
    b = torch.randn(N, generator=g).to(gpu, BF16)
    ref = torch.empty(M, N, device=gpu, dtype=F32)
    _pair(ops, hi, lo, w, b, ref)
    out = torch.full((M, N), float("nan"), device=gpu, dtype=F32)
    ops.linear_skinny(hi, lo, [(w, b, out)])
    assert torch.equal(out, ref)
    out2 = torch.empty_like(out)
    ops.linear_skinny(hi, lo, [(w, b, out2)])
    assert torch.equal(out, out2)                                # bitwise repeat


def test_skinny_gemm_grouped_signed_zeros_and_views(ops, gpu):
    """Two problems per launch at the double block's table shape (28 x 18432 x 3072 x 2). Zero weight rows make exact zeros whose sign
    depends on the epilogue's operation order ((acc + 0)·1 + (acc + bias)·1); outputs are row-strided views with guard columns."""
    M, N, K = 28, 18432, 3072
    hi, lo = _split(ops, gpu, M, K, 3)
    g = torch.Generator().manual_seed(11)
    ws, bs = [], []
    for i in range(2):
        w = torch.randn(N, K, generator=g) * 0.05
        b = torch.randn(N, generator=g)
        w[5 + i :: 97] = 0.0
        b[5 + i :: 194] = 0.0
        b[102 + i :: 194] = -0.0
        ws.append(w.to(gpu, BF16))
        bs.append(b.to(gpu, BF16))
    ref = [torch.empty(M, N, device=gpu, dtype=F32) for _ in range(2)]
    ops.linear_grouped([ops.LinearProblem(hi, ws[0], ref[0], bias=bs[0]), ops.LinearProblem(hi, ws[1], ref[1], bias=bs[1])])
    ops.linear_grouped([ops.LinearProblem(lo, ws[0], ref[0], res=ref[0]), ops.LinearProblem(lo, ws[1], ref[1], res=ref[1])])
    full = [torch.full((M, N + 16), 123.0, device=gpu, dtype=F32) for _ in range(2)]
    ops.linear_skinny(hi, lo, [(ws[0], bs[0], full[0][:, :N]), (ws[1], bs[1], full[1][:, :N])])
    for f, r in zip(full, ref):
        assert torch.equal(f[:, :N].contiguous().view(torch.int32), r.view(torch.int32))     # bit patterns: -0.0 != +0.0 here
        assert bool((f[:, N:] == 123.0).all())                                              # nothing written past N


@pytest.mark.parametrize("xdt", [F32, BF16])
@pytest.mark.parametrize("B,T,N,d", [(1, 512, 4096, 3072), (2, 64, 250, 512), (1, 3, 5, 3072)])
def test_layernorm_pair_equals_two_launches(ops, gpu, xdt, B, T, N, d):
    g = torch.Generator().manual_seed(B + T + N + d)
    x = (torch.randn(B, T + N, d, generator=g) * 3.0 + 0.5).to(gpu, xdt)
    mi, mt = torch.randn(B, 6 * d, generator=g).to(gpu), torch.randn(B, 6 * d, generator=g).to(gpu)
    ch = lambda m, i: m[:, i * d : (i + 1) * d]
    ref = torch.zeros(B, T + N, d, device=gpu, dtype=BF16)
    ops.layernorm_modulate(x[:, T:], ref[:, T:], ch(mi, 3), ch(mi, 4))
    ops.layernorm_modulate(x[:, :T], ref[:, :T], ch(mt, 0), ch(mt, 1))
    out = torch.zeros_like(ref)
    ops.layernorm_modulate_pair(x[:, T:], out[:, T:], ch(mi, 3), ch(mi, 4), x[:, :T], out[:, :T], ch(mt, 0), ch(mt, 1))
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


def _small_model(gpu, guidance=True):
    from oracle import flux_oracle as orc
    from reptext_amd.transformer import FluxTransformer2DModel

    cfg = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=4,
               joint_attention_dim=256, pooled_projection_dim=64, guidance_embeds=guidance, axes_dims_rope=(16, 56, 56))
    tr = FluxTransformer2DModel(**cfg, device=gpu, dtype=BF16)
    tr.load_state_dict(orc.init_mmdit_params(cfg, 1))
    return tr


def _table_the_old_way(ops, mmdit, tr, timesteps, guidance, pooled):
    """What build_modulation_table did before: time_text_embed per step, then the hi / lo pair of launches per block."""
    doubles, singles = tr._ensure_plans()
    B, d, dev = pooled.shape[0], tr.inner_dim, pooled.device
    sc = SimpleNamespace(B=B, temb=torch.empty(B, d, device=dev, dtype=F32), tmp=torch.empty(B, d, device=dev, dtype=F32))
    temb_all = torch.empty(len(timesteps) * B, d, device=dev, dtype=F32)
    for i, t in enumerate(timesteps):
        ts = torch.full((B,), float(t), device=dev, dtype=F32)
        temb_all[i * B : (i + 1) * B].copy_(tr._temb(sc, ts, guidance, pooled))
    hi, lo = ops.silu_split(temb_all, apply_silu=True)
    tabs = []
    ws = [(p.w, p.b) for pl in doubles for p in (pl.ada_img, pl.ada_txt)] + [(pl.ada.w, pl.ada.b) for pl in singles]
    ws.append((tr.norm_out.linear.weight.data, tr.norm_out.linear.bias.data))
    for w, b in ws:
        o = torch.empty(temb_all.shape[0], w.shape[0], device=dev, dtype=F32)
        _pair(ops, hi, lo, w, b, o)
        tabs.append(o)
    return temb_all, tabs


@pytest.mark.parametrize("B,steps,guidance", [(1, 28, True), (2, 9, True), (1, 5, False), (3, 20, True)])
def test_modulation_table_and_temb_all_equal_the_old_way(ops, gpu, B, steps, guidance):
    """steps·B <= 32 takes the skinny GEMM, (3, 20) the general one: both must give the old table."""
    from reptext_amd import mmdit

    tr = _small_model(gpu, guidance)
    g = torch.Generator().manual_seed(B * 100 + steps)
    pooled = torch.randn(B, 64, generator=g).to(gpu, BF16)
    gd = torch.full((B,), 3.5, device=gpu, dtype=F32) if guidance else None
    timesteps = [1.0 - 0.93 * i / steps for i in range(steps)]
    temb_ref, tabs_ref = _table_the_old_way(ops, mmdit, tr, timesteps, gd, pooled)

    ts = torch.tensor([float(t) for t in timesteps for _ in range(B)], device=gpu, dtype=F32)
    t1000, g1000 = tr._embed_scalars(B, ts, gd)
    temb_new = mmdit.time_text_embed_all(tr.time_text_embed, t1000, g1000, pooled, B)
    assert torch.equal(temb_new.view(torch.int32), temb_ref.view(torch.int32))

    tab = tr.build_modulation_table(timesteps, gd, pooled)
    new = [t for pair in tab.double for t in pair] + list(tab.single) + [tab.out]
    assert len(new) == len(tabs_ref)
    for a, b in zip(new, tabs_ref):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    sm = tab.step(steps - 1)
    assert torch.equal(sm.single[0], tabs_ref[4][(steps - 1) * B :])
