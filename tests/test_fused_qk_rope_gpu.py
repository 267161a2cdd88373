"""q/k RMSNorm + RoPE inside the QKV GEMM's epilogue (ops.QKRope) against GEMM followed by qk_rmsnorm_rope on the same inputs:
torch.equal on the WHOLE output buffer (v, MLP and guard columns included) — the fused form stores the same bf16 value through
LDS and runs the same device function, so the acceptance is identity, not a tolerance. Then the denoise loop with the switch
on and off, eager and replayed, and the two-pass path an IP-Adapter forces."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BF16, F32 = torch.bfloat16, torch.float32
SMALL_T = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=4,
               joint_attention_dim=256, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
SMALL_CN = dict(SMALL_T, num_layers=2, num_single_layers=0, extra_condition_channels=64)


@pytest.fixture(scope="module")
def ops(gpu):
    import reptext_amd.ops as ops

    return ops


def _tables(gpu, S, g):
    ang = torch.rand(S, 64, generator=g) * 6.283
    return torch.cos(ang).repeat_interleave(2, dim=1).contiguous().to(gpu), torch.sin(ang).repeat_interleave(2, dim=1).contiguous().to(gpu)


def _norm_w(gpu, g):
    return (1.0 + 0.3 * torch.randn(128, generator=g)).to(gpu, BF16)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("B,S,d,spike", [(1, 4608, 3072, False), (2, 300, 512, False), (1, 700, 512, True)])
def test_single_block_layout_equals_gemm_then_pass(ops, gpu, B, S, d, spike):
    """[k|v|q|mlp] = 7d columns, GELU from 3d on. (1, 4608, 3072) is the benchmark's launch (4608 x 21504 x 3072); (2, 300, 512) is
    ragged (M % 256 != 0) with two batch entries; `spike` puts one huge activation into a row so the sum of squares is not benign."""
    H = d // 128
    g = torch.Generator().manual_seed(S + d)
    x = torch.randn(B, S, d, generator=g)
    if spike:
        x[0, 5, 7] = 300.0
        x[0, 517, 100] = -250.0
    x = x.to(gpu, BF16)
    w = (torch.randn(7 * d, d, generator=g) * 0.04).to(gpu, BF16)
    b = torch.randn(7 * d, generator=g).to(gpu, BF16)
    nq, nk = _norm_w(gpu, g), _norm_w(gpu, g)
    cos, sin = _tables(gpu, S, g)
    ref = torch.full((B, S, 7 * d + 8), 7.0, device=gpu, dtype=BF16)             # 8 guard columns behind the rows
    ops.linear(x, w, ref[..., : 7 * d], bias=b, gelu_from=3 * d)
    ops.qk_rmsnorm_rope(ref, 2 * d, 0, H, 0, None, None, nq, nk, cos, sin)
    out = torch.full_like(ref, 7.0)
    rope = ops.QKRope(2 * d, 0, d, nq, nk, cos, sin)
    ops.linear(x, w, out[..., : 7 * d], bias=b, gelu_from=3 * d, rope=rope)
    assert _same_bits(out, ref)
    out2 = torch.full_like(ref, 7.0)
    ops.linear(x, w, out2[..., : 7 * d], bias=b, gelu_from=3 * d, rope=rope)
    assert _same_bits(out2, out)                                                   # bitwise repeat


@pytest.mark.parametrize("B,T,N,d", [(1, 512, 4096, 3072), (2, 64, 250, 512)])
def test_double_block_grouped_equals_gemm_then_pass(ops, gpu, B, T, N, d):
    """Image and text rows as two groups of one launch ((4096 + 512) x 9216 x 3072 in the benchmark), distinct norm weights per
    stream, image rows at table position T."""
    H, S = d // 128, T + N
    g = torch.Generator().manual_seed(T + N + d)
    x = torch.randn(B, S, d, generator=g).to(gpu, BF16)
    wi, wt = [(torch.randn(3 * d, d, generator=g) * 0.04).to(gpu, BF16) for _ in range(2)]
    bi, bt = [torch.randn(3 * d, generator=g).to(gpu, BF16) for _ in range(2)]
    nqi, nki, nqt, nkt = [_norm_w(gpu, g) for _ in range(4)]
    cos, sin = _tables(gpu, S, g)
    P = ops.LinearProblem
    ref = torch.zeros(B, S, 3 * d, device=gpu, dtype=BF16)
    ops.linear_grouped([P(x[:, T:], wi, ref[:, T:], bias=bi), P(x[:, :T], wt, ref[:, :T], bias=bt)])
    ops.qk_rmsnorm_rope(ref, 0, d, H, T, nqt, nkt, nqi, nki, cos, sin)
    out = torch.zeros_like(ref)
    ops.linear_grouped([P(x[:, T:], wi, out[:, T:], bias=bi, rope=ops.QKRope(0, d, d, nqi, nki, cos, sin, pos0=T)),
                        P(x[:, :T], wt, out[:, :T], bias=bt, rope=ops.QKRope(0, d, d, nqt, nkt, cos, sin, pos0=0))])
    assert _same_bits(out, ref)


def _pipe(gpu, seed):
    from oracle import flux_oracle as orc
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=BF16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=BF16)
    tr.load_state_dict(orc.init_mmdit_params(SMALL_T, seed))
    cn.load_state_dict(orc.init_mmdit_params(SMALL_CN, seed + 1, controlnet=True))
    pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _inputs(gpu, seed):
    from PIL import Image

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu, BF16)
    masks = []
    for box in ((40, 120, 30, 200), (140, 220, 60, 240)):
        m = np.zeros([256, 256], dtype=np.uint8); m[box[0]:box[1], box[2]:box[3]] = 255
        masks.append(Image.fromarray(m))
    return dict(prompt_embeds=r(1, 64, 256), pooled_prompt_embeds=r(1, 64), control_image=[r(1, 256, 128), r(1, 256, 128)], latents=r(1, 256, 64),
                height=256, width=256, num_inference_steps=3, guidance_scale=3.5, control_mask=masks, controlnet_conditioning_step=2, output_type="latent")


def _count_passes(monkeypatch):
    import reptext_amd.ops as ops

    calls = []
    real = ops.qk_rmsnorm_rope
    monkeypatch.setattr(ops, "qk_rmsnorm_rope", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_denoise_loop_is_bitwise_the_same_with_and_without_the_fused_step(gpu, monkeypatch):
    """The small configuration of the graph-replay test (two text lines, tower off after step 2 of 3): latents with the fused step
    equal those of the two-pass path, eager and replayed from the captured graph; the switch is part of the graph signature."""
    from reptext_amd import mmdit

    pipe = _pipe(gpu, 81)
    kw = _inputs(gpu, 82)
    calls = _count_passes(monkeypatch)
    monkeypatch.setattr(mmdit, "FUSED_QK_ROPE", False)
    pipe.capture_graphs = False
    ref = pipe(**kw).images.clone()
    assert len(calls) == 3 * (2 + 2) + 2 * 2 * 2          # every block of the transformer (3 steps) and the tower (2 lines, 2 steps)
    del calls[:]
    monkeypatch.setattr(mmdit, "FUSED_QK_ROPE", True)
    assert torch.equal(pipe(**kw).images, ref)              # eager, fused
    assert not calls                                        # the pass is gone from the loop
    pipe.capture_graphs = True
    assert torch.equal(pipe(**kw).images, ref)              # signature remembered
    assert torch.equal(pipe(**kw).images, ref)              # captured + replayed
    assert torch.equal(pipe(**kw).images, ref)
    n_graphs = len([v for v in pipe._graph_cache.values() if isinstance(v, dict)])
    assert n_graphs == 1
    monkeypatch.setattr(mmdit, "FUSED_QK_ROPE", False)      # another signature: not served by the fused graph
    assert torch.equal(pipe(**kw).images, ref)
    assert torch.equal(pipe(**kw).images, ref)
    assert len([v for v in pipe._graph_cache.values() if isinstance(v, dict)]) == 2


def test_ip_adapter_blocks_take_the_two_pass_path(gpu, monkeypatch):
    """rt_ip_attention reads the raw q, so a double block with an active adapter keeps GEMM + pass; single blocks stay fused."""
    import ip_adapter_reference as ipr
    from reptext_amd import mmdit

    pipe = _pipe(gpu, 91)
    kw = dict(_inputs(gpu, 92), controlnet_conditioning_step=0)
    pipe.load_ip_adapter(ipr.init_ip_params(SMALL_T, n_tokens=4, embed_dim=64, seed=93))
    pipe.set_ip_adapter_scale([1.0, 0.0])                   # block 1 launches nothing for the adapter
    emb = torch.randn(1, 64, generator=torch.Generator().manual_seed(94)).to(gpu, BF16)
    pipe.capture_graphs = False
    monkeypatch.setattr(mmdit, "FUSED_QK_ROPE", False)
    ref = pipe(**kw, ip_adapter_image_embeds=emb).images.clone()
    monkeypatch.setattr(mmdit, "FUSED_QK_ROPE", True)
    calls = _count_passes(monkeypatch)
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=emb).images, ref)
    assert len(calls) == 3                                  # double block 0 of each of the 3 steps
