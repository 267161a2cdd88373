"""CPU tests of the repaint pipeline (reptext_amd/pipeline_repaint.py): the ``t_start`` rule, the mask's way to the packed latent
grid, the refusals (before any native call), the ``__call__`` signature, the unchanged ``CallExtensions``, the shim, and that nothing
of a call — failed or successful — is left on the pipeline. The successful call runs with the loop replaced by a recorder, the way
test_call_extensions_host.py does it: what the loop receives (start state, begin index, the ``Repaint`` record) is checked here, the
loop itself on the GPU. No kernel runs here.

``t_start = int(max(n − min(n·strength, n), 0))`` is the rule (diffusers' ``get_timesteps``, recalled). For (n, strength) = (10, 0.05)
it gives int(9.5) = 9 and leaves ONE step, not zero; a strength that leaves zero steps under this rule is 0 (n·strength = 0), and that
one is refused. Both are pinned below."""
import dataclasses
import inspect
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_true_cfg_host import BASE_PARAMS, CFG, assert_no_call_state, no_native_call  # noqa: E402,F401

H = W = 64
N = 16
BF16 = torch.bfloat16


def _pipe():
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**CFG, device="cpu", dtype=BF16)
    pipe = FluxControlNetRepaintPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, None)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _box(top, bottom, left, right):
    m = np.zeros([H, W], dtype=np.uint8)
    m[top:bottom, left:right] = 255
    return Image.fromarray(m)


def _kw(B=1, **more):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    kw = dict(prompt_embeds=torch.zeros(B, 8, 64, dtype=BF16), pooled_prompt_embeds=torch.zeros(B, 32, dtype=BF16), height=H, width=W,
              num_inference_steps=4, image=r(B, N, 64), mask_image=_box(16, 48, 0, 32), latents=r(B, N, 64).to(BF16), strength=0.75,
              output_type="latent")
    kw.update(more)
    return kw


def test_known_answers_of_the_t_start_rule():
    from reptext_amd.pipeline_repaint import repaint_t_start

    assert repaint_t_start(4, 0.75) == 1                     # 3 of 4 steps run
    assert repaint_t_start(28, 0.6) == 11                    # 28 − 16.8 = 11.2: 17 of 28
    assert repaint_t_start(28, 1.0) == 0
    assert repaint_t_start(10, 0.05) == 9                    # int(9.5): one step is left (see the module docstring)
    assert repaint_t_start(10, 0.1) == 9 and repaint_t_start(1, 1.0) == 0 and repaint_t_start(3, 0.5) == 1
    for n in (1, 10, 28):
        with pytest.raises(ValueError, match="number of pipeline steps is 0"):
            repaint_t_start(n, 0.0)                          # zero steps left
    for bad in (-0.1, 1.01, 2, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            repaint_t_start(28, bad)


def test_the_scheduler_rule_of_the_start_state():
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler

    sc = FlowMatchEulerDiscreteScheduler()
    sc.set_timesteps(sigmas=[1.0, 0.75, 0.5, 0.25], mu=0.6)
    g = torch.Generator().manual_seed(0)
    x, noise = torch.randn(5, 7, generator=g), torch.randn(5, 7, generator=g)
    sigma = float(sc.sigmas[2])
    want = sigma * noise + (1.0 - sigma) * x
    assert torch.equal(sc.scale_noise(x, sigma, noise), want)
    assert torch.equal(sc.scale_noise(x, sc.timesteps[2], noise), want)          # a timestep of the schedule: its sigma
    assert torch.equal(sc.scale_noise(x, 1.0, noise), noise) and torch.equal(sc.scale_noise(x, 0.0, noise), x)
    assert float(sc.sigmas[0]) == 1.0                                            # the schedule starts at pure noise


def test_mask_packing_is_nearest_resize_then_pack():
    pipe = _pipe()
    g = torch.Generator().manual_seed(1)
    pixels = (torch.rand(H, W, generator=g) > 0.5).numpy().astype(np.uint8) * 255        # a binary mask with structure at every scale
    got = pipe._pack_mask(Image.fromarray(pixels), H, W, "cpu")
    m = torch.from_numpy(pixels)[None, None].float() / 255.0
    want = pipe._pack_latents(F.interpolate(m, size=(8, 8), mode="nearest").repeat(1, 16, 1, 1), 1, 16, 8, 8)
    assert got.shape == (1, N, 64) and got.dtype == torch.float32 and torch.equal(got, want)
    assert set(got.unique().tolist()) == {0.0, 1.0}
    assert all(torch.equal(got[0, :, c], got[0, :, c % 4]) for c in range(64))           # the 16 channels carry the same mask
    # grey values are binarised at 0.5 before the resize; another size is resized to the call's first
    grey = Image.fromarray(np.full([H, W], 127, dtype=np.uint8)), Image.fromarray(np.full([2 * H, 2 * W], 128, dtype=np.uint8))
    assert float(pipe._pack_mask(grey[0], H, W, "cpu").max()) == 0.0 and float(pipe._pack_mask(grey[1], H, W, "cpu").min()) == 1.0
    # a packed mask is taken as it is, fractional values included
    soft = torch.rand(1, N, 64, generator=g)
    assert torch.equal(pipe._pack_mask(soft, H, W, "cpu"), soft)
    # no mask_image: the pixel-wise maximum of the control_mask images
    a, b = _box(0, 16, 0, 64), _box(32, 64, 16, 48)
    union = pipe._union_of_masks([a, b])
    assert np.array_equal(np.array(union), np.maximum(np.array(a), np.array(b)))
    rgb = pipe._union_of_masks([a.convert("RGB"), b])                                    # another mode of the same size: taken as grey
    assert np.array_equal(np.array(rgb), np.array(union))


@pytest.mark.parametrize("bad, match", [
    (dict(strength=1.5), "strength"), (dict(strength=-0.01), "strength"), (dict(strength=0.0), "number of pipeline steps"),
    (dict(mask_image=None), "mask_image"), (dict(mask_image=None, control_mask=[]), "mask_image"),
    (dict(mask_image=None, control_mask=[torch.zeros(1, N, 1)]), "token masks"),
    (dict(mask_image=None, control_mask=torch.zeros(1, N, 1)), "list of images"),            # one tensor, not a list: no ambiguous-truth error
    (dict(mask_image=None, control_mask=[Image.new("L", (W, H)), Image.new("L", (W // 2, H))]), "of one size"),
    (dict(mask_image=None, control_mask=[Image.new("L", (W, H)), np.zeros([H, W, 3], dtype=np.uint8)]), "single-channel"),
    (dict(image=None), "image"), (dict(image=torch.zeros(2, N, 64)), "Cannot duplicate `image` of batch size 2 to 3"),
    (dict(image=torch.zeros(3, N + 1, 64)), "`image`: packed latents"), (dict(mask_image=torch.zeros(1, N, 64)[:, :3]), "`mask_image`: packed"),
    (dict(mask_image=torch.zeros(2, N, 64)), "`mask_image`: batch 2"), (dict(image=Image.new("RGB", (W, H))), "needs the pipeline's VAE"),
    (dict(latents=torch.zeros(2, N, 64)), "the noise"),
])
def test_refusals_before_any_device_work(no_native_call, bad, match):
    pipe = _pipe()
    with pytest.raises(ValueError, match=match):
        pipe(**_kw(B=3, **bad))
    assert_no_call_state(pipe)
    assert not {"_repaint", "_repaint_call", "_strength", "_mask_image", "_image"} & set(pipe.__dict__)


def test_the_shim_imports():
    import pipeline_flux_controlnet_repaint as shim
    from reptext_amd import pipeline_repaint

    assert shim.FluxControlNetRepaintPipeline is pipeline_repaint.FluxControlNetRepaintPipeline
    assert shim.repaint_t_start is pipeline_repaint.repaint_t_start
    assert sorted(shim.__all__) == shim.__all__ and "FluxControlNetRepaintPipeline" in shim.__all__


def test_signature_is_the_base_plus_three_and_the_record_is_unchanged():
    from reptext_amd.pipeline import CallExtensions, FluxControlNetPipeline, LoopExtras, Repaint
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline

    params = inspect.signature(FluxControlNetRepaintPipeline.__call__).parameters
    assert list(params) == BASE_PARAMS + ["image", "mask_image", "strength"]
    assert list(inspect.signature(FluxControlNetPipeline.__call__).parameters) == BASE_PARAMS
    base = inspect.signature(FluxControlNetPipeline.__call__).parameters
    assert all(params[k].default == base[k].default for k in BASE_PARAMS[1:])
    assert (params["image"].default, params["mask_image"].default, params["strength"].default) == (None, None, 0.6)
    fields = [f.name for f in dataclasses.fields(CallExtensions)]
    assert len(fields) == 13 and not set(fields) & set(params) and not {"image", "mask_image", "strength"} & set(fields)
    extras = dataclasses.fields(LoopExtras)
    assert {f.name: f.default for f in extras}["repaint"] is None and LoopExtras().repaint is None
    assert [f.name for f in dataclasses.fields(Repaint)] == ["src32", "noise32", "mask"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        Repaint(None, None, None).mask = 1
    # the base pipeline does not take the three names
    from test_true_cfg_host import _kw as base_kw, _pipe as base_pipe
    for name in ("image", "mask_image", "strength"):
        with pytest.raises(TypeError, match=name):
            base_pipe()(**base_kw(), **{name: None})


def test_a_successful_call_hands_the_loop_its_start_and_leaves_nothing_behind():
    from reptext_amd.pipeline import LoopExtras, Repaint

    pipe = _pipe()
    seen = []

    def recorder(latents, *args, **kwargs):
        seen.append((latents, args, kwargs, pipe.scheduler._begin_index))
        pipe._master_latents = latents
        return latents

    pipe._denoise_eager = recorder
    kw = _kw(B=2, mask_image=None, control_mask=[_box(0, 16, 0, 64), _box(32, 64, 16, 48)], true_cfg_scale=2.0,
             negative_prompt_embeds=torch.ones(2, 8, 64, dtype=BF16), negative_pooled_prompt_embeds=torch.ones(2, 32, dtype=BF16))
    out = pipe(**kw)
    assert len(seen) == 1 and out.images.shape == (2, N, 64)
    latents, args, kwargs, begin = seen[0]
    x = kwargs["extras"]
    assert isinstance(x, LoopExtras) and isinstance(x.repaint, Repaint) and x.cfg_scale == 2.0
    assert begin == 1 and pipe.num_timesteps == 3 and len(args[4]) == 3                 # tvals: the last 3 of 4 steps
    full = pipe.scheduler.timesteps.tolist()
    assert args[4] == full[1:] and args[13] == 3 and len(pipe.scheduler.sigmas) == 5    # the grid is the base's, cut
    rp = x.repaint
    assert rp.src32.shape == rp.noise32.shape == (2, N, 64) and rp.mask.shape == (1, N, 64)                # not doubled under CFG
    assert rp.src32.dtype == rp.noise32.dtype == rp.mask.dtype == latents.dtype == torch.float32
    assert args[0].shape == (4, 8, 64)                                                   # the conditioning is
    assert torch.equal(rp.src32, kw["image"]) and torch.equal(rp.noise32, kw["latents"].float())
    sigma = float(pipe.scheduler.sigmas[1])
    assert torch.equal(latents, sigma * rp.noise32 + (1.0 - sigma) * rp.src32)           # scale_noise at the first sigma that runs
    assert torch.equal(rp.mask, pipe._pack_mask(pipe._union_of_masks(kw["control_mask"]), H, W, "cpu"))
    rows = rp.mask[0, :, 0].reshape(4, 4)                                                # 4x4 tokens of 16 pixels
    assert rows.tolist() == [[1, 1, 1, 1], [0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 1, 0]]
    assert_no_call_state(pipe)
    assert not {"_repaint", "_repaint_call", "_strength", "_mask_image", "_image"} & set(pipe.__dict__)
    # strength 1: every step, from pure noise; one source for a batch of two
    seen.clear()
    pipe(**dict(kw, strength=1.0, image=kw["image"][:1]))
    latents, args, kwargs, begin = seen[0]
    assert begin == 0 and len(args[4]) == 4 and torch.equal(latents, kw["latents"].float())
    assert torch.equal(kwargs["extras"].repaint.src32, kw["image"][:1].expand(2, -1, -1))
    # a base-style call afterwards starts at step 0 again
    seen.clear()
    from reptext_amd.pipeline import FluxControlNetPipeline
    FluxControlNetPipeline.__call__(pipe, **{k: v for k, v in kw.items() if k not in ("image", "mask_image", "strength")})
    assert seen[0][3] is None and seen[0][2]["extras"].repaint is None and len(seen[0][1][4]) == 4
    assert_no_call_state(pipe)
