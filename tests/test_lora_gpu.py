"""GPU tests of the LoRA path: rt_lora_merge_bf16 against an fp64 CPU reference, model parity with merged adapters against the fp32
oracle, and the pipeline contract (call scale, captured graphs, unload / unfuse restore, fp8 plans, inpaint)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402

SMALL_T = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=4,
               joint_attention_dim=256, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
SMALL_CN = dict(SMALL_T, num_layers=2, num_single_layers=1, extra_condition_channels=64)


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def assert_at_dtype_floor(err_fp32, err_stored, floor):
    """Restated from test_models_gpu.py: GPU vs fp32 oracle, GPU vs bf16-storage oracle, bf16-storage oracle vs fp32 oracle."""
    assert err_fp32 <= 1.25 * floor + 1e-4, (err_fp32, floor)
    assert err_stored <= 1.45 * floor + 1e-4, (err_stored, floor)


def _ordered(x):
    """bf16 bit patterns as integers ordered like the values (adjacent representable values differ by 1)."""
    i = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _check_bf16(out, ref64, mag64):
    """Within 1 bf16 ulp of bf16(fp64 result) and >= 99.9 % equal to it. Where W0 and the delta cancel, the result is far smaller
    than its operands and the fp32 accumulation's own error (2^-24 of |W0| + Σ|c·B·A|) can exceed an ulp of that tiny result:
    those elements are held to that fp32 floor instead (2^-20, i.e. 16x its size)."""
    ref = ref64.to(torch.float32).to(torch.bfloat16)
    out = out.cpu()
    d = (_ordered(out) - _ordered(ref)).abs()
    ok = (d <= 1) | ((out.double() - ref64).abs() <= mag64 * 2.0 ** -20)
    assert bool(ok.all()), (int(d.max()), int((~ok).sum()))
    assert float((d == 0).double().mean()) >= 0.999, float((d == 0).double().mean())


def _reference(w0_rows, terms, rows):
    """fp64 W0 + Σ c·B·A on the sampled rows (c as the fp32 coefficient the ABI takes), and the magnitude |W0| + Σ|c|·|B|·|A|."""
    ref, mag = w0_rows.cpu().double(), w0_rows.cpu().double().abs()
    for B, At, c in terms:
        c32 = float(torch.tensor(c, dtype=torch.float32))
        b, a = B[rows].cpu().double(), At.cpu().double()
        ref += c32 * (b @ a.t())
        mag += abs(c32) * (b.abs() @ a.abs().t())
    return ref, mag


def _factors(N, K, r, gen, dev):
    r_pad = (r + 31) // 32 * 32
    B = torch.zeros(N, r_pad, dtype=torch.bfloat16)
    At = torch.zeros(K, r_pad, dtype=torch.bfloat16)
    B[:, :r] = (torch.randn(N, r, generator=gen) * 0.05).to(torch.bfloat16)
    At[:, :r] = (torch.randn(K, r, generator=gen) * 0.05).to(torch.bfloat16)
    return B.to(dev), At.to(dev)


SHAPES = [(64, 3072), (3072, 64), (3072, 256), (3072, 768), (3072, 3072), (6144, 3072), (9216, 3072), (12288, 3072), (18432, 3072),
          (3072, 4096), (3072, 12288), (3072, 15360), (100, 72)]
# (ranks, scales) per case: 1-4 terms, every rank of {1, 4, 16, 64, 128, 200} (200 -> r_pad 224, an odd number of 32-wide steps),
# negative and zero scales, a different scale on every term (a kernel that reused one term's scale or dropped a term fails)
TERM_CASES = [([200], [0.7]),
              ([64, 1], [-1.3, 0.45]),
              ([4, 200, 16], [0.7, 0.0, -1.9]),
              ([128, 64, 200, 1], [2.5, -1.3, 0.0, 0.3])]
KERNEL_CASES = [(N, K, c) for i, (N, K) in enumerate(SHAPES) for c in (i % 4, (i + 2) % 4)]


@pytest.mark.parametrize("N, K, case", KERNEL_CASES)
def test_merge_kernel_matches_fp64(gpu, N, K, case):
    """Out of place and in place; every element within 1 bf16 ulp of bf16(fp64 result) (or the fp32 floor where W0 and the delta
    cancel, see _check_bf16) and >= 99.9 % equal to it, on a row sample that includes both edges. No terms: W0's bits."""
    from reptext_amd import ops

    ranks, scales = TERM_CASES[case]
    gen = torch.Generator().manual_seed(N * 7 + K + 1000 * case)
    w0 = (torch.randn(N, K, generator=gen) * 0.02).to(torch.bfloat16).to(gpu)
    terms = [(*_factors(N, K, r, gen, gpu), c) for r, c in zip(ranks, scales)]
    rows = torch.unique(torch.cat([torch.randint(0, N, (160,), generator=gen), torch.tensor([0, N - 1])]))
    ref, mag = _reference(w0[rows], terms, rows)
    out = torch.empty_like(w0)
    ops.lora_merge_(out, w0, terms)
    _check_bf16(out[rows], ref, mag)
    ops.lora_merge_(w0, w0, terms)                                             # in place
    assert torch.equal(w0, out)
    cp = torch.full_like(w0, 7.0)
    ops.lora_merge_(cp, w0, [])                                                # no terms: W0's bits
    assert torch.equal(cp, w0)


def test_merge_entry_rejects_bad_arguments_on_real_buffers(gpu):
    """The host checks of rt_lora_merge_bf16 that need non-null pointers, on real device buffers sized so that even a launch would
    stay inside them (the null-pointer checks are in test_lora_host.py)."""
    from reptext_amd import native

    lib = native.load()
    big = torch.zeros(256, 256, device=gpu, dtype=torch.bfloat16)
    fac = torch.zeros(256, 256, device=gpu, dtype=torch.bfloat16)
    P, F = big.data_ptr(), fac.data_ptr()
    t = (native.LoraTerm * 9)()
    for i in range(9):
        t[i] = native.LoraTerm(F, F, 256, 256, 32, 1.0)
    call = lambda terms, n, W0=P, ld0=64, W=P, ldw=64, N=64, K=64: lib.rt_lora_merge_bf16(terms, n, W0, ld0, W, ldw, N, K, None)
    assert call(t, 9) == -3                                                    # RT_E_SHAPE: more than RT_LORA_MAX_TERMS
    assert call(t, 1, K=60) == -3                                              # K % 8
    assert call(t, 1, N=0) == -1
    assert call(t, 1, ld0=32) == -1                                            # ld0 < K
    assert call(t, 1, W=P + 8) == -2                                           # RT_E_ALIGN
    assert call(t, 1, ld0=68) == -2
    bad = (native.LoraTerm * 1)(native.LoraTerm(F, F, 256, 256, 48, 1.0))
    assert call(bad, 1) == -3                                                  # r_pad % 32
    bad[0] = native.LoraTerm(F + 4, F, 256, 256, 32, 1.0)
    assert call(bad, 1) == -2
    bad[0] = native.LoraTerm(F, F, 16, 256, 32, 1.0)                           # ldb < r_pad
    assert call(bad, 1) == -1
    torch.cuda.synchronize()
    assert not big.any() and not fac.any()                                     # nothing was launched


def test_merge_kernel_row_view_of_fused_storage(gpu):
    """to_k inside the fused [q|k|v] storage: rows d..2d merged in place, the rest untouched."""
    from reptext_amd import ops

    d = 3072
    gen = torch.Generator().manual_seed(3)
    qkv = (torch.randn(3 * d, d, generator=gen) * 0.02).to(torch.bfloat16).to(gpu)
    before = qkv.clone()
    B, At = _factors(d, d, 64, gen, gpu)
    ops.lora_merge_(qkv[d:2 * d], before[d:2 * d], [(B, At, -0.8)])
    assert torch.equal(qkv[:d], before[:d]) and torch.equal(qkv[2 * d:], before[2 * d:])
    rows = torch.arange(0, d, 37)
    _check_bf16(qkv[d:2 * d][rows], *_reference(before[d:2 * d][rows], [(B, At, -0.8)], rows))


def _lora_sd(params, gen, r=16, alpha=24.0, only=None, prefix=""):
    """Random rank-r adapter with per-module alpha on every Linear of an oracle parameter dict."""
    sd = {}
    for k, w in params.items():
        if not k.endswith(".weight") or w.dim() != 2:
            continue
        path = k[: -len(".weight")]
        if only is not None and path not in only:
            continue
        out_f, in_f = w.shape
        sd[f"{prefix}{path}.lora_A.weight"] = (torch.randn(r, in_f, generator=gen) / in_f ** 0.5).to(torch.bfloat16)
        sd[f"{prefix}{path}.lora_B.weight"] = (torch.randn(out_f, r, generator=gen) * 0.02).to(torch.bfloat16)
        sd[f"{prefix}{path}.alpha"] = torch.tensor(alpha)
    return sd


def _merged_params(params, sd, scale=1.0, prefix=""):
    """The oracle's weights with the adapter merged in fp64 and rounded to bf16 once."""
    out = dict(params)
    for k in sd:
        if not k.endswith(".lora_A.weight"):
            continue
        path = k[len(prefix): -len(".lora_A.weight")]
        A, B = sd[k].double(), sd[prefix + path + ".lora_B.weight"].double()
        sigma = float(sd[prefix + path + ".alpha"]) / A.shape[0]
        w = params[path + ".weight"].double() + scale * sigma * (B @ A)
        out[path + ".weight"] = w.to(torch.float32).to(torch.bfloat16).to(torch.float32)
    return out


def _inputs(B, T, h2, w2, seed):
    g = torch.Generator().manual_seed(seed)
    N = (h2 // 2) * (w2 // 2)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    return dict(latents=r(B, N, 64), cond=r(B, N, 128), prompt=r(B, T, 256), pooled=r(B, 64), img_ids=orc.latent_image_ids(h2, w2),
                txt_ids=torch.zeros(T, 3), timestep=torch.full((B,), 0.622459), guidance=torch.full((B,), 3.5))


def test_model_parity_with_merged_adapters(gpu):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.transformer import FluxTransformer2DModel

    tp = orc.init_mmdit_params(SMALL_T, seed=41)
    cp = orc.init_mmdit_params(SMALL_CN, seed=42, controlnet=True)
    gen = torch.Generator().manual_seed(43)
    sd_t = _lora_sd(tp, gen, prefix="transformer.")
    sd_c = _lora_sd(cp, gen, r=8, alpha=8.0, only={"transformer_blocks.0.attn.to_q", "controlnet_blocks.1", "x_embedder"})
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(tp)
    cn.load_state_dict(cp)
    x = _inputs(1, 64, 16, 24, seed=44)
    d = {k: (v.to(gpu, torch.bfloat16) if k in ("latents", "cond", "prompt", "pooled", "img_ids", "txt_ids") else v.to(gpu)) for k, v in x.items()}
    kw = dict(encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["timestep"], img_ids=d["img_ids"],
              txt_ids=d["txt_ids"], guidance=d["guidance"], return_dict=False)
    base = tr(hidden_states=d["latents"], **kw)[0].float().cpu()
    tr.load_lora_adapter(sd_t, adapter_name="t")
    cn.load_lora_adapter(sd_c, adapter_name="c")
    assert tr.active_adapters() == ["t"] and cn.active_adapters() == ["c"]
    out = tr(hidden_states=d["latents"], **kw)[0].float().cpu()
    targs = (x["latents"], x["prompt"], x["pooled"], x["timestep"], x["img_ids"], x["txt_ids"])
    tpm = _merged_params(tp, sd_t, prefix="transformer.")
    ref = orc.transformer_forward(tpm, SMALL_T, *targs, guidance=x["guidance"])
    with orc.stored_as(torch.bfloat16):
        ref16 = orc.transformer_forward(tpm, SMALL_T, *targs, guidance=x["guidance"])
    err, err16, floor = rel_l2(out, ref), rel_l2(out, ref16), rel_l2(ref16, ref)
    print(f"transformer + LoRA: rel-L2 {err:.3e} vs fp32 oracle, {err16:.3e} vs bf16-storage oracle (floor {floor:.3e}); "
          f"adapter moves the output by {rel_l2(out, base):.3e}")
    assert_at_dtype_floor(err, err16, floor)
    assert rel_l2(out, base) >= 10 * floor                                     # the merge really happened
    # the tower, with a call scale of 0.5 (CN:263-276)
    bs, ss = cn(hidden_states=d["latents"], controlnet_cond=d["cond"], conditioning_scale=0.8, joint_attention_kwargs={"scale": 0.5}, **kw)
    cpm = _merged_params(cp, sd_c, scale=0.5)
    cargs = (x["latents"], x["cond"], x["prompt"], x["pooled"], x["timestep"], x["img_ids"], x["txt_ids"])
    rb, rs = orc.controlnet_forward(cpm, SMALL_CN, *cargs, guidance=x["guidance"], conditioning_scale=0.8)
    with orc.stored_as(torch.bfloat16):
        rb16, rs16 = orc.controlnet_forward(cpm, SMALL_CN, *cargs, guidance=x["guidance"], conditioning_scale=0.8)
    for a, b, b16 in zip(bs + ss, rb + rs, rb16 + rs16):
        assert_at_dtype_floor(rel_l2(a.float().cpu(), b), rel_l2(a.float().cpu(), b16), rel_l2(b16, b))
    with pytest.raises(RuntimeError, match="unload"):
        tr.load_state_dict(tp)
    tr.unload_lora()
    assert torch.equal(tr(hidden_states=d["latents"], **kw)[0].float().cpu(), base)


def _pipe(gpu, seed, inpaint=False):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16).random_init_(seed)
    cn = FluxControlNetModel(**dict(SMALL_CN, num_single_layers=0), device=gpu, dtype=torch.bfloat16).random_init_(seed + 1)
    if inpaint:
        from reptext_amd.pipeline_inpaint import FluxControlNetPipeline

        cni = FluxControlNetModel(**dict(SMALL_CN, num_single_layers=0, extra_condition_channels=4), device=gpu,
                                  dtype=torch.bfloat16).random_init_(seed + 2)
        pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn, cni)
    else:
        from reptext_amd.pipeline import FluxControlNetPipeline

        pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _pipe_inputs(gpu, seed):
    from PIL import Image

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu, torch.bfloat16)
    m = np.zeros([256, 256], dtype=np.uint8)
    m[40:120, 30:200] = 255
    return dict(prompt_embeds=r(1, 64, 256), pooled_prompt_embeds=r(1, 64), control_image=[r(1, 256, 128)], latents=r(1, 256, 64),
                height=256, width=256, num_inference_steps=3, guidance_scale=3.5, control_mask=[Image.fromarray(m)],
                controlnet_conditioning_step=2, output_type="latent")


def _weights(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def test_pipeline_lora_contract(gpu):
    import reptext_amd.pipeline as P

    pipe = _pipe(gpu, 81)
    kw = _pipe_inputs(gpu, 82)
    gen = torch.Generator().manual_seed(83)
    params = {k: v.float().cpu() for k, v in pipe.transformer.state_dict().items()}
    sd_a, sd_b = _lora_sd(params, gen, prefix="transformer."), _lora_sd(params, gen, r=4, alpha=4.0)
    w_before = _weights(pipe.transformer)
    # a graph captured BEFORE the load replays the merged weights
    pipe.capture_graphs = False
    base = pipe(**kw).images.clone()
    pipe.capture_graphs = True
    pipe(**kw)
    assert torch.equal(pipe(**kw).images, base)                               # captured + replayed
    assert len([v for v in pipe._graph_cache.values() if isinstance(v, dict)]) == 1
    pipe.load_lora_weights(sd_a, adapter_name="a")
    assert pipe.get_active_adapters() == ["a"] and pipe.get_list_adapters() == {"transformer": ["a"]}
    replayed = pipe(**kw).images.clone()
    pipe.capture_graphs = False
    eager1 = pipe(**kw).images.clone()
    assert torch.equal(replayed, eager1) and not torch.equal(eager1, base)
    # joint_attention_kwargs={"scale": s} == set_adapters(a, s), and the next call without kwargs is weight 1.0 again
    half = pipe(**kw, joint_attention_kwargs={"scale": 0.5}).images.clone()
    assert torch.equal(pipe(**kw).images, eager1)
    pipe.set_adapters("a", 0.5)
    assert torch.equal(pipe(**kw).images, half)
    pipe.set_adapters("a", 1.0)
    # scale-only kwargs are served by the graph (no eager loop runs)
    pipe.capture_graphs = True
    calls = []
    orig = pipe._denoise_eager
    pipe._denoise_eager = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    assert torch.equal(pipe(**kw, joint_attention_kwargs={"scale": 0.5}).images, half)
    assert torch.equal(pipe(**kw).images, eager1)
    assert calls == []
    del pipe._denoise_eager
    pipe.capture_graphs = False
    # fuse then unfuse, a second adapter, delete: restore bit for bit
    pipe.load_lora_weights(sd_b, adapter_name="b")
    pipe.set_adapters(["a", "b"], [0.7, -0.3])
    two = pipe(**kw).images.clone()
    pipe.fuse_lora(adapter_names=["a"])
    assert torch.equal(pipe(**kw).images, two)
    with pytest.raises(ValueError, match="already fused"):
        pipe.fuse_lora(adapter_names=["a"])
    pipe.unfuse_lora()
    assert torch.equal(pipe(**kw).images, two)
    pipe.disable_lora()
    assert torch.equal(pipe(**kw).images, base)
    pipe.enable_lora()
    pipe.delete_adapters("b")
    pipe.set_adapters("a")
    assert torch.equal(pipe(**kw).images, eager1)
    # state_dict() between calls holds the weights at call scale 1.0, even right after a scaled call
    pipe(**kw, joint_attention_kwargs={"scale": 0.5})
    sd_after_scaled = _weights(pipe.transformer)
    pipe(**kw)
    assert all(torch.equal(v, sd_after_scaled[k]) for k, v in pipe.transformer.state_dict().items())
    # unload: every weight and the no-LoRA output come back bit for bit
    pipe.unload_lora_weights()
    assert all(torch.equal(v, w_before[k]) for k, v in pipe.transformer.state_dict().items())
    assert torch.equal(pipe(**kw).images, base)
    assert pipe.get_list_adapters() == {}
    # fuse_lora() + unload_lora_weights() keeps the fused adapter in the weights (diffusers' recipe); unfused ones are dropped
    pipe.load_lora_weights(sd_a, adapter_name="a")
    pipe.load_lora_weights(sd_b, adapter_name="b")
    pipe.set_adapters(["a", "b"], [1.0, -0.3])
    pipe.fuse_lora(adapter_names=["a"])
    pipe.unload_lora_weights()
    assert getattr(pipe.transformer, "_lora", None) is None
    assert torch.equal(pipe(**kw).images, eager1)                              # a at weight 1.0, baked in; b gone
    pipe.transformer.load_state_dict(w_before)                                  # allowed again once unloaded
    assert torch.equal(pipe(**kw).images, base)


@pytest.mark.parametrize("level", ["ln", "mx"])
def test_fp8_plans_are_requantised_in_place(gpu, level):
    pipe = _pipe(gpu, 91)
    kw = _pipe_inputs(gpu, 92)
    tr = pipe.transformer
    tr.enable_fp8_linears(level)
    gen = torch.Generator().manual_seed(93)
    sd = _lora_sd({k: v.float().cpu() for k, v in tr.state_dict().items()}, gen)
    pipe.capture_graphs = True
    pipe(**kw)
    pipe(**kw)                                                                 # captured
    plans = tr._ensure_plans()
    tr.load_lora_adapter(sd, adapter_name="a")
    assert tr._ensure_plans() is plans                                         # same plans, same buffers
    replayed = pipe(**kw).images.clone()
    rows = tr._fp8_rows()
    # 2 double blocks x (q|k|v of both streams + ff.net.0 of both) + 2 single blocks x (k|v|q|proj_mlp), and under "mx" also the
    # out / ff.net.2 projections and proj_out; the adapter targets every Linear, so each of them is requantised
    assert len(rows) == {"ln": 2 * 8 + 2 * 4, "mx": 2 * 12 + 2 * 5}[level]
    copies = {p: (w8[r0:r1].clone(), ws[r0:r1].clone()) for p, (_, w8, ws, r0, r1) in rows.items()}
    tr._plans = None                                                           # fresh plans from the merged bf16 weights
    fresh = tr._fp8_rows()
    assert fresh is not rows and sorted(fresh) == sorted(copies)
    for p, (_, w8, ws, r0, r1) in fresh.items():
        assert torch.equal(copies[p][0].view(torch.uint8), w8[r0:r1].view(torch.uint8)) and torch.equal(copies[p][1], ws[r0:r1]), p
    pipe.capture_graphs = False
    assert torch.equal(pipe(**kw).images, replayed)


def test_inpaint_pipeline_with_adapter_and_scale(gpu):
    pipe = _pipe(gpu, 101, inpaint=True)
    kw = _pipe_inputs(gpu, 102)
    g = torch.Generator().manual_seed(103)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu, torch.bfloat16)
    kw.update(negative_prompt_embeds=r(1, 64, 256), negative_pooled_prompt_embeds=r(1, 64), true_guidance_scale=2.0,
              control_image_inpaint=r(1, 256, 68), controlnet_conditioning_scale_inpaint=1.0)
    base = pipe(**kw).images.clone()
    sd = _lora_sd({k: v.float().cpu() for k, v in pipe.transformer.state_dict().items()}, torch.Generator().manual_seed(104),
                  only={"transformer_blocks.0.attn.to_q", "single_transformer_blocks.1.proj_out"})
    pipe.load_lora_weights(sd)
    half = pipe(**kw, joint_attention_kwargs={"scale": 0.5}).images.clone()
    assert torch.isfinite(half).all() and not torch.equal(half, base)
    pipe.set_adapters(pipe.get_active_adapters(), 0.5)
    assert torch.equal(pipe(**kw).images, half)
    pipe.unload_lora_weights()
    assert torch.equal(pipe(**kw).images, base)
