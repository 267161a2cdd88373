"""GPU tests of the IP-Adapter path: rt_ip_attention against an fp32 CPU reference, the transformer and the pipeline with an adapter
against the tests' fp32 restatement (tests/ip_adapter_reference.py), and the pipeline contract (no embeds / zero scales / unload are
bitwise the no-adapter result; the captured loop is kept, its embeds are a static input and its scales part of the key)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ip_adapter_reference as ipr  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402

from oracle import flux_oracle as orc  # noqa: E402

SMALL_T = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=4,
               joint_attention_dim=256, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
SMALL_CN = dict(SMALL_T, num_layers=2, num_single_layers=0, extra_condition_channels=64)
E = 64


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def assert_at_dtype_floor(err_fp32, err_stored, floor):
    """Restated from test_models_gpu.py: GPU vs fp32 oracle, GPU vs storage-precision oracle, that oracle vs the fp32 one."""
    assert err_fp32 <= 1.25 * floor + 1e-4, (err_fp32, floor)
    assert err_stored <= 1.45 * floor + 1e-4, (err_stored, floor)


# ------------------------------------------------------------------------------------------------------------------ the kernel
# (n_ip, N, H, B, shared K/V, fp32 o, accumulate, fused q|k|v row). Every n_ip of {1, 4, 16, 17, 100, 128}, N of {4096, 4160, 3844, 37},
# H of {4, 24}, B of {1, 3} appears, each n_ip with both o dtypes and both accumulate settings somewhere.
KERNEL_CASES = [
    (1, 37, 4, 1, True, False, False, True),
    (1, 4160, 24, 1, True, True, True, False),
    (4, 4096, 24, 1, True, False, False, True),
    (4, 3844, 4, 3, False, True, True, True),
    (4, 37, 4, 3, True, False, True, False),
    (16, 4160, 4, 3, False, False, True, True),
    (16, 4096, 24, 1, True, True, False, False),
    (17, 3844, 24, 1, True, False, True, True),
    (17, 37, 4, 3, False, True, False, True),
    (100, 4096, 4, 3, False, False, False, True),
    (100, 4160, 24, 1, True, True, True, True),
    (128, 3844, 4, 3, True, False, True, False),
    (128, 4096, 24, 1, False, True, False, True),
    (128, 37, 4, 1, True, False, False, True),
]


def _kernel_inputs(n_ip, N, H, B, shared, seed, key_std=1.5):
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16)
    mag = 10.0 ** (torch.rand(B, N, 1, 1, generator=g) * 2.0 - 1.0)           # raw query rows spread over two decades
    q = bf(torch.randn(B, N, H, 128, generator=g) * mag)
    wq = bf(torch.rand(128, generator=g) + 0.5)                                # U(0.5, 1.5)
    Bk = 1 if shared else B
    k = bf(torch.randn(Bk, n_ip, H, 128, generator=g) * key_std)
    v = bf(torch.randn(Bk, n_ip, H, 128, generator=g))
    return q, wq, k, v


@pytest.mark.parametrize("n_ip, N, H, B, shared, o_f32, accumulate, fused", KERNEL_CASES)
def test_ip_attention_kernel_matches_fp32(gpu, n_ip, N, H, B, shared, o_f32, accumulate, fused):
    """rel_l2 < 5e-3 against the fp32 CPU reference from the same bf16 inputs (the bound test_kernels_gpu.py holds the bf16
    attention kernels to). Before the GPU is compared the reference itself shows that every step of the math is visible in these
    inputs: a kernel that skipped the softmax, the RMSNorm, norm_q.weight or the mask of the padded keys would be >= 0.1 away
    (>= 0.03 for the padding at n_ip = 100: twelve stray keys among a hundred move less)."""
    from reptext_amd import ops

    d = H * 128
    q, wq, k, v = _kernel_inputs(n_ip, N, H, B, shared, seed=1000 * n_ip + N + H + B)
    ip_scale = -1.3 if (n_ip + N) % 2 else 0.7
    ref = ipr.ip_attention_ref(q, wq, k, v, ip_scale)
    wrong = lambda **kw: rel_l2(ipr.ip_attention_ref(q, wq, k, v, ip_scale, **kw), ref)
    if n_ip >= 4:
        vis = dict(uniform=wrong(uniform=True), no_norm=wrong(norm=False), no_wq=wrong(weight=False))
        print(f"n_ip={n_ip} N={N} H={H} B={B}: wrong-answer distances {vis}")
        assert vis["uniform"] >= 0.1 and vis["no_norm"] >= 0.1 and vis["no_wq"] >= 0.1, vis
    if n_ip % 16:
        pad = wrong(pad_keys_to=(n_ip + 15) // 16 * 16)
        print(f"n_ip={n_ip}: unmasked padding distance {pad:.3f}")
        assert pad >= (0.03 if n_ip == 100 else 0.1), pad

    # device buffers: q inside a wider row (the fused q|k|v buffer, or 8 spare columns), o with spare rows and columns as canaries
    ldq = 3 * d if fused else d + 8
    qbuf = torch.randn(B, N, ldq).to(torch.bfloat16)
    qbuf[..., :d] = q.reshape(B, N, d)
    qdev = qbuf.to(gpu)
    q_before = qdev.clone()
    ldo, rows_o = d + 16, N + 3
    odt = torch.float32 if o_f32 else torch.bfloat16
    obuf = (torch.randn(B, rows_o, ldo) * 0.5).to(odt)
    odev = obuf.to(gpu)
    kdev, vdev = k.reshape(-1, n_ip, d).to(gpu), v.reshape(-1, n_ip, d).to(gpu)
    ops.ip_attention(qdev[..., :d], wq.to(gpu), kdev, vdev, odev[:, :N, :d], H, ip_scale=ip_scale, accumulate=accumulate)
    torch.cuda.synchronize()
    out = odev.cpu()
    want = ref + obuf[:, :N, :d].float() if accumulate else ref
    err = rel_l2(out[:, :N, :d].float(), want)
    print(f"n_ip={n_ip} N={N} H={H} B={B} shared={shared} o_f32={o_f32} accumulate={accumulate} ldq={ldq}: rel_l2 {err:.3e}")
    assert err < 5e-3, err
    assert torch.equal(qdev, q_before)                                          # q is not modified
    assert torch.equal(out[:, N:], obuf[:, N:]) and torch.equal(out[:, :, d:], obuf[:, :, d:])     # canaries: rows >= N, columns >= H*128


def test_ip_attention_rejects_bad_arguments_on_real_buffers(gpu):
    from reptext_amd import ops

    q = torch.zeros(1, 64, 512, device=gpu, dtype=torch.bfloat16)
    wq = torch.ones(128, device=gpu, dtype=torch.bfloat16)
    o = torch.zeros_like(q)
    kv = lambda n, b=1: torch.zeros(b, n, 512, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="1..128"):
        ops.ip_attention(q, wq, kv(129), kv(129), o, 4)
    with pytest.raises(ValueError, match="batch 1 or B"):
        ops.ip_attention(q, wq, kv(4, 2), kv(4, 2), o, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ip_attention(q.cpu(), wq, kv(4), kv(4), o, 4)
    torch.cuda.synchronize()
    assert not o.any()


# ------------------------------------------------------------------------------------------------------------------ the model
def _inputs(B, T, h2, w2, seed):
    g = torch.Generator().manual_seed(seed)
    N = (h2 // 2) * (w2 // 2)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    return dict(latents=r(B, N, 64), prompt=r(B, T, 256), pooled=r(B, 64), img_ids=orc.latent_image_ids(h2, w2), txt_ids=torch.zeros(T, 3),
                timestep=torch.full((B,), 0.622459), guidance=torch.full((B,), 3.5), samples=[r(B, N, 512) * 0.5, r(B, N, 512) * 0.5],
                embeds=r(B, E))


def _model_case(gpu, n_tokens, scales, seed, B=1, fp8=False, fp8_attn=False, shared_embeds=False):
    from reptext_amd.transformer import FluxTransformer2DModel

    tp = orc.init_mmdit_params(SMALL_T, seed=seed)
    ipp = ipr.init_ip_params(SMALL_T, n_tokens=n_tokens, embed_dim=E, seed=seed + 1)
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(tp)
    if fp8:
        tr.enable_fp8_linears(fp8)
    if fp8_attn:
        tr.enable_fp8_attention(True)
    tr.load_ip_adapter(ipp if seed % 2 else ipr.to_xlabs(ipp))
    tr.set_ip_adapter_scale(scales)
    x = _inputs(B, 64, 32, 32, seed=seed + 2)                                  # N = 256, T = 64
    emb = x["embeds"][:1] if shared_embeds else x["embeds"]
    b16 = lambda t: t.to(gpu, torch.bfloat16)
    kw = dict(hidden_states=b16(x["latents"]), encoder_hidden_states=b16(x["prompt"]), pooled_projections=b16(x["pooled"]),
              timestep=x["timestep"].to(gpu), img_ids=b16(x["img_ids"]), txt_ids=b16(x["txt_ids"]), guidance=x["guidance"].to(gpu),
              controlnet_block_samples=[b16(s) for s in x["samples"]], return_dict=False)
    targs = (tp, SMALL_T, x["latents"], x["prompt"], x["pooled"], x["timestep"], x["img_ids"], x["txt_ids"])
    okw = dict(guidance=x["guidance"], controlnet_block_samples=x["samples"])
    ikw = dict(ip_params=ipp, ip_embeds=emb, ip_scales=scales)
    return tr, kw, b16(emb), targs, okw, ikw


def _check_model(tr, kw, emb, targs, okw, ikw, contexts, min_ratio, label):
    import contextlib

    ref = ipr.transformer_forward(*targs, **okw, **ikw)
    with contextlib.ExitStack() as st:
        for c in contexts:
            st.enter_context(c())
        ref_s = ipr.transformer_forward(*targs, **okw, **ikw)
    without = ipr.transformer_forward(*targs, **okw)
    floor, moved = rel_l2(ref_s, ref), rel_l2(ref, without)
    print(f"{label}: floor {floor:.3e}, with-against-without {moved:.3e} (ratio {moved / floor:.1f})")
    assert moved >= min_ratio * floor, (moved, floor)                           # condition on the oracle: the term cannot hide
    out = tr(**kw, joint_attention_kwargs={"ip_adapter_image_embeds": emb})[0].float().cpu()
    err, err_s = rel_l2(out, ref), rel_l2(out, ref_s)
    print(f"{label}: GPU rel-L2 {err:.3e} vs fp32 restatement, {err_s:.3e} vs storage-precision restatement")
    assert_at_dtype_floor(err, err_s, floor)
    return out


@pytest.mark.parametrize("n_tokens, scales, B, shared", [(4, [1.0, -0.7], 1, False), (16, [0.6, -1.2], 2, False), (16, [0.0, 0.9], 2, True),
                                                         (4, [-0.8, 0.0], 1, False)])
def test_transformer_with_adapter_and_controlnet_samples(gpu, n_tokens, scales, B, shared):
    tr, kw, emb, targs, okw, ikw = _model_case(gpu, n_tokens, scales, seed=200 + n_tokens + B, B=B, shared_embeds=shared)
    out = _check_model(tr, kw, emb, targs, okw, ikw, [lambda: orc.stored_as(torch.bfloat16)], 10, f"bf16 n={n_tokens} scales={scales}")
    # the kwargs path equals the prepared path bitwise; without embeds, or at scale 0, the output is the no-adapter one bitwise
    prepared = tr._ip_adapter.prepare(emb)
    assert torch.equal(tr(**kw, _ip=prepared)[0].float().cpu(), out)
    jk = {"ip_adapter_image_embeds": [emb[:, None]]}
    assert torch.equal(tr(**kw, joint_attention_kwargs=jk)[0].float().cpu(), out)
    assert list(jk) == ["ip_adapter_image_embeds"]                              # popped from a copy: the caller's dict is as it was
    plain = tr(**kw)[0].float().cpu()
    assert not torch.equal(plain, out)
    tr.set_ip_adapter_scale(0.0)
    assert torch.equal(tr(**kw, joint_attention_kwargs={"ip_adapter_image_embeds": emb})[0].float().cpu(), plain)
    tr.unload_ip_adapter()
    assert torch.equal(tr(**kw)[0].float().cpu(), plain)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        tr(**kw, joint_attention_kwargs={"ip_adapter_image_embeds": emb})


def test_transformer_with_adapter_without_controlnet_samples(gpu):
    """No sample: the term itself rides the add2 slot of the ff2 epilogue instead of the accumulate pass."""
    tr, kw, emb, targs, okw, ikw = _model_case(gpu, 4, [1.0, -0.7], seed=231)
    kw2 = dict(kw, controlnet_block_samples=None)
    okw2 = dict(okw, controlnet_block_samples=None)
    _check_model(tr, kw2, emb, targs, okw2, ikw, [lambda: orc.stored_as(torch.bfloat16)], 10, "no samples")


@pytest.mark.parametrize("level, attn", [("ln", False), ("mx", False), ("mx", True), ("ln", True)])
def test_transformer_with_adapter_fp8_modes(gpu, level, attn):
    """As test_models_gpu.py compares those modes: against the restatement under stored_as(bf16) + fp8_linears(level)
    [+ fp8_attention()], the floor being that run's distance from fp32. orc.linear quantises by module name, so the adapter's own
    linears stay bf16 on both sides."""
    tr, kw, emb, targs, okw, ikw = _model_case(gpu, 16, [1.0, -0.7], seed=240, B=2, fp8=level, fp8_attn=attn)
    ctx = [lambda: orc.stored_as(torch.bfloat16), lambda: orc.fp8_linears(level)] + ([lambda: orc.fp8_attention()] if attn else [])
    _check_model(tr, kw, emb, targs, okw, ikw, ctx, 3, f"fp8 {level} attention={attn}")


# ------------------------------------------------------------------------------------------------------------------ the pipeline
def _pipe(gpu, seed, inpaint=False):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tp, cp = orc.init_mmdit_params(SMALL_T, seed), orc.init_mmdit_params(SMALL_CN, seed + 1, controlnet=True)
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=torch.bfloat16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=torch.bfloat16)
    tr.load_state_dict(tp)
    cn.load_state_dict(cp)
    if inpaint:
        from reptext_amd.pipeline_inpaint import FluxControlNetPipeline

        cni = FluxControlNetModel(**dict(SMALL_CN, extra_condition_channels=4), device=gpu, dtype=torch.bfloat16).random_init_(seed + 2)
        pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn, cni)
    else:
        from reptext_amd.pipeline import FluxControlNetPipeline

        pipe = FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    return pipe, tp, cp


def _pipe_inputs(gpu, seed, steps=2):
    from PIL import Image

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    H = W = 256
    N, T = 256, 64
    cpu = dict(pe=r(1, T, 256), pooled=r(1, 64), hint=r(1, N, 128), lat0=orc.pack_latents(r(1, 16, 32, 32)), embeds=r(1, E), embeds2=r(1, E))
    m = np.zeros([H, W], dtype=np.uint8)
    m[60:140, 80:200] = 255
    cpu["mask"] = torch.nn.functional.interpolate(torch.from_numpy(m)[None, None].float() / 255.0, scale_factor=1 / 16, mode="bilinear").reshape(1, -1, 1)
    b16 = lambda t: t.to(gpu, torch.bfloat16)
    kw = dict(prompt_embeds=b16(cpu["pe"]), pooled_prompt_embeds=b16(cpu["pooled"]), height=H, width=W, num_inference_steps=steps, guidance_scale=3.5,
              control_image=[b16(cpu["hint"])], control_mask=[Image.fromarray(m)], controlnet_conditioning_scale=1.0,
              controlnet_conditioning_step=30, latents=b16(cpu["lat0"]), output_type="latent")
    return kw, cpu


def test_pipeline_two_steps_with_tower_masks_and_adapter(gpu):
    pipe, tp, cp = _pipe(gpu, 301)
    kw, c = _pipe_inputs(gpu, 302)
    pipe.capture_graphs = False
    base = pipe(**kw).images.clone()
    ipp = ipr.init_ip_params(SMALL_T, n_tokens=4, embed_dim=E, seed=303)
    scales = [1.0, -0.7]
    pipe.load_ip_adapter(ipp)
    pipe.set_ip_adapter_scale(scales)
    emb = c["embeds"].to(gpu, torch.bfloat16)
    assert torch.equal(pipe(**kw).images, base)                                 # no embeds: bitwise the no-adapter result
    out = pipe(**kw, ip_adapter_image_embeds=[emb[:, None]]).images.float().cpu()
    sig = orc.flow_sigmas(2, orc.calculate_shift(256, 256, 4096, 0.5, 1.15))
    largs = (tp, SMALL_T, cp, SMALL_CN, c["lat0"], c["pe"], c["pooled"], [c["hint"]], [c["mask"]], sig, orc.latent_image_ids(32, 32), torch.zeros(64, 3), 3.5)
    ikw = dict(ip_params=ipp, ip_embeds=c["embeds"], ip_scales=scales)
    ref = ipr.denoise_loop(*largs, **ikw)
    with orc.stored_as(torch.bfloat16):
        ref16 = ipr.denoise_loop(*largs, **ikw)
    without = orc.denoise_loop(*largs)
    floor, moved = rel_l2(ref16, ref), rel_l2(ref, without)
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"pipeline + adapter: rel-L2 {err:.3e} vs fp32 loop, {err16:.3e} vs bf16-storage loop (floor {floor:.3e}); the adapter moves the "
          f"latents by {moved:.3e}")
    assert moved >= 10 * floor
    assert_at_dtype_floor(err, err16, floor)
    assert torch.equal(pipe(**kw, joint_attention_kwargs={"ip_adapter_image_embeds": emb}).images.float().cpu(), out)
    assert_no_call_state(pipe)
    pipe.set_ip_adapter_scale(0.0)
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=emb).images, base)   # all scales 0
    pipe.set_ip_adapter_scale(1.0)
    pipe.unload_ip_adapter()
    assert torch.equal(pipe(**kw).images, base)
    pipe.unload_ip_adapter()                                                    # a second unload is harmless
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe(**kw, ip_adapter_image_embeds=emb)
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
        pipe(**kw, ip_adapter_image=object())


def test_pipeline_graph_with_adapter(gpu):
    pipe, tp, cp = _pipe(gpu, 311)
    kw, c = _pipe_inputs(gpu, 312, steps=3)
    ipp = ipr.init_ip_params(SMALL_T, n_tokens=16, embed_dim=E, seed=313)
    pipe.load_ip_adapter(ipr.to_xlabs(ipp))
    pipe.set_ip_adapter_scale([0.8, -0.5])
    e1, e2 = c["embeds"].to(gpu, torch.bfloat16), c["embeds2"].to(gpu, torch.bfloat16)
    pipe.capture_graphs = False
    eager1 = pipe(**kw, ip_adapter_image_embeds=e1).images.clone()
    eager2 = pipe(**kw, ip_adapter_image_embeds=e2).images.clone()
    base = pipe(**kw).images.clone()
    assert not torch.equal(eager1, eager2) and not torch.equal(eager1, base)
    pipe.capture_graphs = True
    calls = []
    orig = pipe._denoise_eager
    pipe._denoise_eager = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e1).images, eager1)  # first sight: eager
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e1).images, eager1)  # captured + replayed
    n_before = len(calls)
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e1).images, eager1)  # replay only
    assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e2).images, eager2)  # new embed VALUES, same signature: replayed, copied in
    assert len(calls) == n_before
    assert len([v for v in pipe._graph_cache.values() if isinstance(v, dict)]) == 1
    # a changed scale is another signature: the old graph is not replayed
    pipe.set_ip_adapter_scale([0.8, 0.3])
    pipe._denoise_eager = orig
    pipe.capture_graphs = False
    eager3 = pipe(**kw, ip_adapter_image_embeds=e1).images.clone()
    assert not torch.equal(eager3, eager1)
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw, ip_adapter_image_embeds=e1).images, eager3)
    # the no-embeds signature still has its own graph and its own result
    for _ in range(3):
        assert torch.equal(pipe(**kw).images, base)


def test_pipeline_adapter_with_lora(gpu):
    from test_lora_gpu import _lora_sd

    pipe, tp, cp = _pipe(gpu, 321)
    kw, c = _pipe_inputs(gpu, 322, steps=2)
    emb = c["embeds"].to(gpu, torch.bfloat16)
    pipe.load_ip_adapter(ipr.init_ip_params(SMALL_T, n_tokens=4, embed_dim=E, seed=323))
    pipe.load_lora_weights(_lora_sd(tp, torch.Generator().manual_seed(324), prefix="transformer."), adapter_name="a")
    pipe.capture_graphs = False
    eager = pipe(**kw, ip_adapter_image_embeds=emb, joint_attention_kwargs={"scale": 0.5}).images.clone()
    only_lora = pipe(**kw, joint_attention_kwargs={"scale": 0.5}).images.clone()
    assert not torch.equal(eager, only_lora)
    pipe.capture_graphs = True
    for _ in range(3):
        assert torch.equal(pipe(**kw, ip_adapter_image_embeds=emb, joint_attention_kwargs={"scale": 0.5}).images, eager)
    assert len([v for v in pipe._graph_cache.values() if isinstance(v, dict)]) == 1
    pipe.unload_lora_weights()
    pipe.unload_ip_adapter()


def test_inpaint_pipeline_refuses_image_prompts(gpu):
    pipe, _, _ = _pipe(gpu, 331, inpaint=True)
    kw, c = _pipe_inputs(gpu, 332)
    emb = c["embeds"].to(gpu, torch.bfloat16)
    with pytest.raises(ValueError, match="IP-Adapter"):
        pipe(**kw, ip_adapter_image_embeds=emb)
    with pytest.raises(ValueError, match="IP-Adapter"):
        pipe(**kw, ip_adapter_image=object())
