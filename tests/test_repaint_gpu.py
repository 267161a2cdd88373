"""The repaint pipeline (reptext_amd/pipeline_repaint.py) on the GPU: parity of the loop with the CPU oracle's (tests/loop_reference.py)
alone, under true CFG and with the union tower; the bitwise properties of the call — the background ends as the source, strength 1 under
a mask of ones is the base call, eager = captured = replay, the base call's graph key is untouched, batch invariance, the loop's toggles —
and one call through the small VAE with PIL inputs. 256x256 (N = 256, T = 64) with the reduced models of test_vae_pipeline_gpu.py, 4
steps of which strength 0.75 runs 3."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as orc  # noqa: E402
from test_models_gpu import assert_at_dtype_floor  # noqa: E402
from test_true_cfg_gpu import BOXES, SMALL_UN, graph_keys, mask_images, negatives, token_mask  # noqa: E402
from test_true_cfg_host import assert_no_call_state  # noqa: E402
from test_vae_pipeline_gpu import SMALL_CN, SMALL_T, rel_l2, vae_pair  # noqa: E402,F401

from loop_reference import denoise_loop_reference  # noqa: E402

H = W = 256
N, T = 256, 64
BOX = (60, 140, 80, 200)                                 # the box of test_pipeline_c1_latents_and_image: rows 48..144 of tokens
BF16 = torch.bfloat16


def box_image(box):
    m = np.zeros([H, W], dtype=np.uint8); m[box[0]:box[1], box[2]:box[3]] = 255
    return Image.fromarray(m)


def random_pipe(gpu, seed, union=False, vae=None):
    """(pipe, r): a repaint pipeline with random transformer and text tower (and union tower); r(*shape) draws bf16 device tensors."""
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=BF16).random_init_(seed)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=BF16).random_init_(seed + 1)
    pipe = FluxControlNetRepaintPipeline(FlowMatchEulerDiscreteScheduler(), vae, None, None, None, None, tr, cn)
    if union:
        pipe.controlnet_union = FluxControlNetModel(**SMALL_UN, device=gpu, dtype=BF16).random_init_(seed + 2)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(seed)
    return pipe, (lambda *s: torch.randn(*s, generator=g).to(gpu, BF16))


def two_line_call(r, steps=4, cn_steps=2, B=1, strength=0.75):
    """Two masked text lines (row window active), the tower on for cn_steps of the steps that run; the mask is the union of the two
    lines' boxes (mask_image=None), the source packed fp32 latents."""
    return dict(prompt_embeds=r(B, T, 256), pooled_prompt_embeds=r(B, 64), height=H, width=W, num_inference_steps=steps, guidance_scale=3.5,
                control_image=[r(B, N, 128), r(B, N, 128)], control_mask=mask_images(BOXES), controlnet_conditioning_step=cn_steps,
                latents=r(B, N, 64), image=r(B, N, 64).float() * 0.5 + 0.123, strength=strength, output_type="latent")


def base_call(pipe, kw):
    from reptext_amd.pipeline import FluxControlNetPipeline

    return FluxControlNetPipeline.__call__(pipe, **{k: v for k, v in kw.items() if k not in ("image", "mask_image", "strength")})


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", ["plain", "cfg", "union", "everything"])
def test_repaint_matches_the_oracle_loop(gpu, case):
    """One masked text line, a box mask, strength 0.75 of 4 steps (3 run, from sigma_1): GPU error at the bf16-storage oracle's own floor.
    The same under true CFG at s = 2 and with the union tower on [0.3, 1.0] of the steps that run (text tower for 2 of them). The
    condition on the inputs — asserted on the oracle alone — is that the loop WITHOUT the blend lies at least 10 floors away.
    ``everything``: every loop extension in one call — true CFG, the union tower, the multistep scheduler and a guider that projects
    on [0, 0.67] (guided at steps 0 and 1 of the 3, its clamp at half the ‖d‖ the reference shows at step 0: active) — and the
    reference also lies at least 10 floors from itself with the guider, the second order or the union tower left out."""
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.guidance import TrueCFGGuider
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline, repaint_t_start
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tp = orc.init_mmdit_params(SMALL_T, seed=811)
    cp = orc.init_mmdit_params(SMALL_CN, seed=812, controlnet=True)
    tr = FluxTransformer2DModel(**SMALL_T, device=gpu, dtype=BF16)
    cn = FluxControlNetModel(**SMALL_CN, device=gpu, dtype=BF16)
    tr.load_state_dict(tp); cn.load_state_dict(cp)
    sched = FlowMatchMultistepScheduler() if case == "everything" else FlowMatchEulerDiscreteScheduler()
    pipe = FluxControlNetRepaintPipeline(sched, None, None, None, None, None, tr, cn)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(813)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16).float()
    pe, pooled, npe, npooled, hint = r(1, T, 256), r(1, 64), r(1, T, 256), r(1, 64), r(1, N, 128)
    npe, npooled = (3 * npe).to(BF16).float(), (3 * npooled).to(BF16).float()          # as in test_true_cfg_matches_the_oracle_loop
    noise = orc.pack_latents(r(1, 16, 32, 32))
    src = torch.randn(1, N, 64, generator=g) * 0.7 + 0.2                                # fp32, not on the bf16 grid
    uhint = r(1, N, 64)
    rm = token_mask(BOX)
    b16 = lambda t: t.to(gpu, BF16)
    cn_steps = 2 if case in ("union", "everything") else 30
    call = dict(prompt_embeds=b16(pe), pooled_prompt_embeds=b16(pooled), height=H, width=W, num_inference_steps=4, guidance_scale=3.5,
                control_image=[b16(hint)], control_mask=[box_image(BOX)], controlnet_conditioning_scale=1.0, controlnet_conditioning_step=cn_steps,
                latents=b16(noise), image=src.to(gpu), mask_image=box_image(BOX), strength=0.75, output_type="latent")
    rkw = dict(conditioning_scale=1.0, conditioning_step=cn_steps)
    if case in ("cfg", "everything"):
        call.update(negative_prompt_embeds=b16(npe), negative_pooled_prompt_embeds=b16(npooled), true_cfg_scale=2.0)
        rkw["negative"] = dict(prompt_embeds=npe, pooled=npooled, scale=2.0)
    if case in ("union", "everything"):
        up = orc.init_mmdit_params(SMALL_UN, seed=814, controlnet=True)
        un = FluxControlNetModel(**SMALL_UN, device=gpu, dtype=BF16)
        un.load_state_dict(up)
        pipe.controlnet_union = un
        call.update(control_image_union=b16(uhint), controlnet_conditioning_scale_union=0.7, control_guidance_start_union=0.3,
                    control_guidance_end_union=1.0)
        rkw["union"] = dict(params=up, cfg=SMALL_UN, cond=uhint, scale=0.7, start=0.3, end=1.0)
    mask = pipe._pack_mask(box_image(BOX), H, W, "cpu")
    assert 0 < int(mask.sum()) < mask.numel() and set(mask.unique().tolist()) == {0.0, 1.0}
    t_start = repaint_t_start(4, 0.75)
    sig = orc.flow_sigmas(4, orc.calculate_shift(N, 256, 4096, 0.5, 1.15))
    args = (tp, SMALL_T, cp, SMALL_CN, noise, pe, pooled, [hint], [rm], sig, orc.latent_image_ids(32, 32), torch.zeros(T, 3), 3.5)
    rkw["repaint"] = dict(src=src, noise=noise, mask=mask, t_start=t_start)
    if case == "everything":
        info = {}                                                   # one step: its d is the plain CFG difference
        denoise_loop_reference(*args[:9], sig[: t_start + 2], *args[10:], **rkw, guider=TrueCFGGuider(eta=0.0), info=info)
        pipe.guider = TrueCFGGuider(stop=0.67, eta=0.0, momentum=-0.5, norm_threshold=0.5 * float(info["norm_d"][0]))
        rkw.update(order=2, guider=pipe.guider)
    ref = denoise_loop_reference(*args, **rkw)
    with orc.stored_as(BF16):
        ref16 = denoise_loop_reference(*args, **rkw)
    unblended = denoise_loop_reference(*args, **{**rkw, "repaint": dict(rkw["repaint"], blend=False)})
    floor, felt = rel_l2(ref16, ref), rel_l2(unblended, ref)
    if case == "everything":
        away = {what: rel_l2(denoise_loop_reference(*args, **{**rkw, **without}), ref) / floor
                for what, without in (("guider", dict(guider=None)), ("second order", dict(order=1)), ("union tower", dict(union=None)))}
        print(f"repaint [{case}] floor {floor:.3e}; the reference without the blend lies {felt / floor:.0f} floors away, without the "
              + ", ".join(f"{what} {d:.0f}" for what, d in away.items()))
        assert min(away.values()) >= 10
    out = pipe(**call).images.float().cpu()
    assert pipe.scheduler._step_index == 4 and len(pipe.scheduler.sigmas) == len(sig)
    err, err16 = rel_l2(out, ref), rel_l2(out, ref16)
    print(f"repaint [{case}] latents rel-L2 {err:.3e} vs fp32 oracle, {err16:.3e} vs bf16-storage oracle (floor {floor:.3e}); the loop "
          f"without the blend lies {felt:.3e} = {felt / floor:.0f} x floor away")
    assert felt >= 10 * floor
    assert_at_dtype_floor(err, err16, floor)
    assert_no_call_state(pipe)


# ------------------------------------------------------------------------------------------------------------------ 1b. the mask's resize
def test_mask_packing_on_the_device_is_the_host_packing(gpu):
    """``_pack_mask`` resizes with ``ops.resize2d(mode="nearest")`` on the device and with ``F.interpolate`` on the host (what
    test_repaint_host.py pins against ``F.interpolate`` + ``_pack_latents``): the same bits, on a mask with structure at every scale, at
    the call's size and at one that is resized to it first, and for a batch of two."""
    pipe, _ = random_pipe(gpu, 815)
    g = torch.Generator().manual_seed(2)
    noise_mask = lambda h, w: Image.fromarray((torch.rand(h, w, generator=g) > 0.5).numpy().astype(np.uint8) * 255)
    for mask in (noise_mask(H, W), noise_mask(H // 2 + 3, W + 10), [noise_mask(H, W), box_image(BOX)]):
        on_device, on_host = pipe._pack_mask(mask, H, W, gpu), pipe._pack_mask(mask, H, W, "cpu")
        assert on_device.is_cuda and on_device.shape == on_host.shape == (len(mask) if isinstance(mask, list) else 1, N, 64)
        assert torch.equal(on_device.cpu(), on_host) and 0 < int(on_host.sum()) < on_host.numel()


# ------------------------------------------------------------------------------------------------------------------ 2. the background
def test_tokens_outside_the_mask_end_as_the_source_bit_for_bit(gpu):
    pipe, r = random_pipe(gpu, 821)
    kw = two_line_call(r, B=2)
    for extra in ({}, dict(**negatives(r, B=2), true_cfg_scale=2.0)):
        out = pipe(**kw, **extra).images
        assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        mask = pipe._pack_mask(pipe._union_of_masks(kw["control_mask"]), H, W, gpu).expand(2, -1, -1)
        assert 0 < int(mask.sum()) < mask.numel()
        assert torch.equal(out[mask == 0], kw["image"][mask == 0])
        assert not bool((out[mask == 1] == kw["image"][mask == 1]).any())
    # a soft mask blends: 0 keeps the source, anything else does not
    soft = torch.rand(1, N, 64, generator=torch.Generator().manual_seed(1)).to(gpu)
    soft[:, : N // 2] = 0.0
    out = pipe(**dict(kw, mask_image=soft)).images
    assert torch.equal(out[:, : N // 2], kw["image"][:, : N // 2]) and not bool((out[:, N // 2:] == kw["image"][:, N // 2:]).any())


# ------------------------------------------------------------------------------------------------------------------ 3. strength 1, mask of ones
def test_full_strength_under_a_mask_of_ones_is_the_base_call(gpu):
    """strength = 1 starts from sigma_0 = 1, where the start state is the noise, and under m = 1 the step is the plain step
    (test_repaint_step_kernel_gpu.py): the base pipeline's call on the same arguments, bit for bit — also under true CFG."""
    pipe, r = random_pipe(gpu, 831)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r, strength=1.0), mask_image=torch.ones(1, N, 64, device=gpu))
    for extra in ({}, dict(**negatives(r), true_cfg_scale=2.0)):
        want = base_call(pipe, {**kw, **extra}).images.clone()
        assert pipe.scheduler._step_index == 4
        got = pipe(**kw, **extra).images
        assert torch.equal(got, want) and pipe.scheduler._step_index == 4
        assert not torch.equal(pipe(**dict(kw, strength=0.75), **extra).images, want)


# ------------------------------------------------------------------------------------------------------------------ 4. eager = captured = replay
def test_repaint_loop_graph_replay_is_bitwise_the_eager_loop_and_the_base_key_stays(gpu):
    pipe, r = random_pipe(gpu, 841)
    kw = two_line_call(r)
    base_first = base_call(pipe, kw).images.clone()                         # seen: the base call's key
    base_keys = graph_keys(pipe)
    assert len(base_keys) == 1 and not any(isinstance(k, tuple) and k[:1] == ("repaint",) for k in base_keys[0])
    pipe.capture_graphs = False
    eager = pipe(**kw).images.clone()
    assert pipe.scheduler._step_index == 4                                  # begin index 1 + 3 steps
    assert graph_keys(pipe) == base_keys
    pipe.capture_graphs = True
    for _ in range(3):                                                      # seen, captured, replayed
        assert torch.equal(pipe(**kw).images, eager)
        assert pipe.scheduler._step_index == 4
    keys = graph_keys(pipe)
    assert len(keys) == 2 and keys[0] == base_keys[0]                       # one new key
    new = [k for k in keys[1] if isinstance(k, tuple) and k[:1] == ("repaint",)]
    assert len(new) == 1 and len(new[0]) == 4 and isinstance(pipe._graph_cache[keys[1]], dict)
    # new source, noise and mask VALUES, same signature: replayed, copied in
    kw2 = dict(kw, image=kw["image"].flip(1).contiguous(), latents=r(1, N, 64), control_mask=mask_images(((48, 96, 30, 200), (100, 150, 90, 240))))
    pipe.capture_graphs = False
    eager2 = pipe(**kw2).images.clone()
    pipe.capture_graphs = True
    assert torch.equal(pipe(**kw2).images, eager2) and not torch.equal(eager2, eager)
    assert graph_keys(pipe) == keys
    # the base call after: its old key, now captured, the same result
    for _ in range(2):
        assert torch.equal(base_call(pipe, kw).images, base_first)
    assert graph_keys(pipe) == keys and pipe.scheduler._step_index == 4
    assert_no_call_state(pipe)


# ------------------------------------------------------------------------------------------------------------------ 5. batch
def test_batch_of_two_with_per_sample_sources_is_two_calls(gpu):
    pipe, r = random_pipe(gpu, 851)
    pipe.capture_graphs = False
    kw = two_line_call(r, B=2)
    kw["control_mask"] = [torch.cat([token_mask(a), token_mask(b)]).to(gpu, BF16) for a, b in
                          (((48, 96, 30, 200), (64, 112, 10, 120)), ((100, 150, 60, 240), (90, 140, 100, 250)))]
    masks = [pipe._pack_mask(box_image(b), H, W, gpu) for b in ((48, 150, 30, 240), (64, 140, 10, 250))]
    kw["mask_image"] = torch.cat(masks)
    both = pipe(**kw).images.clone()
    assert not torch.equal(both[0], both[1])
    per_sample = ("control_image", "control_mask")
    for b in range(2):
        one = {k: (v[b : b + 1] if isinstance(v, torch.Tensor) else [t[b : b + 1] for t in v] if k in per_sample else v) for k, v in kw.items()}
        assert torch.equal(pipe(**one).images, both[b : b + 1]), b


# ------------------------------------------------------------------------------------------------------------------ 6. toggles
def test_overlap_and_row_window_are_bitwise_neutral_for_a_repaint(gpu, monkeypatch):
    import reptext_amd.pipeline as P

    pipe, r = random_pipe(gpu, 861, union=True)
    pipe.capture_graphs = False
    kw = dict(two_line_call(r, steps=4, cn_steps=3), control_image_union=r(1, N, 64), controlnet_conditioning_scale_union=0.7,
              control_guidance_start_union=0.2, control_guidance_end_union=0.8)
    monkeypatch.setattr(P, "OVERLAP_TOWER", False)
    serial = pipe(**kw).images.clone()
    assert pipe._tower_window_used is not None
    monkeypatch.setattr(P, "OVERLAP_TOWER", True)
    assert torch.equal(pipe(**kw).images, serial)
    monkeypatch.setattr(P, "TOWER_WINDOW", False)
    for overlap in (False, True):
        monkeypatch.setattr(P, "OVERLAP_TOWER", overlap)
        assert torch.equal(pipe(**kw).images, serial)
        assert pipe._tower_window_used is None


# ------------------------------------------------------------------------------------------------------------------ 7. end to end
def test_call_with_pil_source_mask_and_hints(vae_pair, gpu):
    """The infer-shaped call through the small VAE: PIL source, PIL mask, PIL hints, an image out. mask_image=None is the union of the
    control_mask images. Draw order: the hints' posteriors from the global RNG, then the source's posterior and the noise from
    ``generator`` — replayed by seeding both before each call."""
    from PIL import ImageDraw

    _, vae = vae_pair
    pipe, r = random_pipe(gpu, 871, vae=vae)
    g = torch.Generator().manual_seed(5)
    photo = Image.fromarray((torch.rand(H, W, 3, generator=g) * 255).to(torch.uint8).numpy())
    edges = Image.new("RGB", (W, H), (255, 255, 255))
    ImageDraw.Draw(edges).rectangle((60, 90, 190, 150), outline=(0, 0, 0))
    boxes = ((85, 155, 55, 195), (170, 220, 30, 120))
    lines = [box_image(b) for b in boxes]
    kw = dict(prompt_embeds=r(1, T, 256), pooled_prompt_embeds=r(1, 64), height=H, width=W, num_inference_steps=4, guidance_scale=3.5,
              control_image=[edges, edges], control_position=lines, control_mask=lines, image=photo, strength=0.75, output_type="np")

    def run(**more):
        torch.manual_seed(1234)
        return pipe(**kw, **more, generator=torch.Generator().manual_seed(42)).images

    default = run()
    assert default.shape == (1, H, W, 3) and bool(np.isfinite(default).all()) and float(default.std()) > 1e-3
    union = Image.fromarray(np.maximum(np.array(lines[0]), np.array(lines[1])))
    assert np.array_equal(run(mask_image=union), default)
    assert not np.array_equal(run(mask_image=lines[0]), default)
    # the latents outside the mask are the encoded source
    lat = pipe(**dict(kw, output_type="latent"), generator=torch.Generator().manual_seed(42)).images
    mask = pipe._pack_mask(union, H, W, gpu)
    src = pipe._source_latents(photo, H, W, gpu, torch.Generator().manual_seed(42))
    assert torch.equal(lat[mask == 0], src[mask == 0])
    assert_no_call_state(pipe)
