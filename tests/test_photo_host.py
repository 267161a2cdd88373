"""CPU tests of the photo pipeline (reptext_amd/pipeline_photo.py): the known answers of ``photo_crop_region``, every refusal (made on
the host, before any native call), the ``__call__`` signature, the shim, that nothing of a call is left on the pipeline, and the fp64
restatements of the kernels (tests/photo_reference.py) against themselves on the cases that are exact. No kernel runs here.

The region's rounding rule, pinned below: the mask's box grows by ``pad`` and is clamped; the side that is too short for the working
aspect becomes ``ceil(other · aspect)``; of the pixels added, ``floor(half)`` go to the left / top; then the box is shifted inside."""
import dataclasses
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from photo_reference import aa_tap_count, composite_ref, gaussian_blur_ref, resize_aa_ref  # noqa: E402
from test_true_cfg_host import BASE_PARAMS, CFG, assert_no_call_state, no_native_call  # noqa: E402,F401

PH, PW = 200, 264                 # the photo
H, W = 64, 96                     # the working size
BF16 = torch.bfloat16


def _pipe():
    from reptext_amd.pipeline_photo import FluxControlNetPhotoPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**CFG, device="cpu", dtype=BF16)
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 2, 3, 4)))        # a VAE is present; no refusal reaches it
    pipe = FluxControlNetPhotoPipeline(FlowMatchEulerDiscreteScheduler(), vae, None, None, None, None, tr, None)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _box(top=80, bottom=120, left=100, right=160, h=PH, w=PW):
    m = np.zeros([h, w], dtype=np.uint8)
    m[top:bottom, left:right] = 255
    return Image.fromarray(m)


def _kw(**more):
    g = torch.Generator().manual_seed(3)
    photo = torch.randint(0, 256, (PH, PW, 3), generator=g, dtype=torch.uint8).numpy()
    kw = dict(prompt_embeds=torch.zeros(1, 8, 64, dtype=BF16), pooled_prompt_embeds=torch.zeros(1, 32, dtype=BF16), height=H, width=W,
              num_inference_steps=4, image=photo, mask_image=_box(), control_image=[Image.new("RGB", (PW, PH), (255, 255, 255))],
              control_mask=[_box()], control_position=[_box()], strength=0.75, padding_mask_crop=16, mask_blur=4.0, output_type="np")
    kw.update(more)
    return kw


def test_known_answers_of_the_crop_region():
    from reptext_amd.pipeline_photo import photo_crop_region as region

    # a box in the middle: (100..160) x (80..120) + 16 -> 92 x 72, too narrow for 96:64 -> 108 wide, 8 added on either side
    assert region((100, 80, 160, 120), PW, PH, 16, 96, 64) == (76, 64, 184, 136)
    # an odd number of added pixels: 93 x 72 -> 108 wide, 15 added, 7 to the left and 8 to the right
    assert region((100, 80, 161, 120), PW, PH, 16, 96, 64) == (77, 64, 185, 136)
    # a box at the corner: clamped to 76 x 56, grown to 84 wide about its centre (x0 = -4) and shifted back inside
    assert region((0, 0, 60, 40), PW, PH, 16, 96, 64) == (0, 0, 84, 56)
    assert region((204, 160, 264, 200), PW, PH, 16, 96, 64) == (180, 144, 264, 200)
    # an aspect that needs widening / heightening, at a photo's scale
    assert region((1000, 1000, 1200, 2400), 4000, 3000, 32, 1024, 1024) == (368, 968, 1832, 2432)
    assert region((1000, 1000, 2200, 1400), 4000, 3000, 32, 1024, 1024) == (968, 568, 2232, 1832)
    assert region((100, 80, 160, 120), PW, PH, 0, 64, 96) == (100, 55, 160, 145)              # 60 wide -> 90 high
    # the region that already has the working size: nothing will be resampled
    assert region((100, 84, 164, 116), PW, PH, 16, 96, 64) == (84, 68, 180, 132)
    # the whole photo
    assert region((10, 10, 20, 20), 96, 64, 100, 96, 64) == (0, 0, 96, 64)
    # a photo too small for the aspect: the error names a working size that fits, and that size does fit
    with pytest.raises(ValueError, match=r"too small .* width=96, height=32"):
        region((10, 10, 250, 60), 264, 100, 16, 64, 96)
    assert region((10, 10, 250, 60), 264, 100, 16, 96, 32) == (0, 0, 264, 88)
    with pytest.raises(ValueError, match="too small"):
        region((0, 0, 96, 10), 96, 64, 0, 64, 96)
    for bad in ((5, 5, 5, 9), (-1, 0, 4, 4), (0, 0, PW + 1, 4)):
        with pytest.raises(ValueError, match="bbox"):
            region(bad, PW, PH, 16, 96, 64)


@pytest.mark.parametrize("bad, match", [
    (dict(mask_image=Image.new("L", (PW, PH)), control_mask=None), "mask is empty"),
    (dict(mask_image=None, control_mask=[Image.new("L", (PW, PH))]), "mask is empty"),
    (dict(mask_image=None, control_mask=None), "mask_image"),
    (dict(padding_mask_crop=11), "smallest padding_mask_crop that works is 12"),
    (dict(padding_mask_crop=0, mask_blur=0.4), "smallest padding_mask_crop that works is 2"),
    (dict(mask_blur=-1.0), "mask_blur"), (dict(mask_blur=40.0, padding_mask_crop=200), "mask_blur"),
    (dict(mask_image=_box(h=PH // 2, w=PW // 2)), "`mask_image`: 132x100 pixels"),
    (dict(control_image=[Image.new("RGB", (W, H))]), r"`control_image\[0\]`: 96x64 pixels, .* the photo's size 264x200"),
    (dict(control_mask=[_box(), _box(h=PH, w=PW - 1)]), r"`control_mask\[1\]`: 263x200"),
    (dict(control_position=[_box(h=H, w=W, top=0, bottom=8, left=0, right=8)]), r"`control_position\[0\]`"),
    (dict(control_glyph=Image.new("RGB", (W, H))), "`control_glyph`"),
    (dict(control_image_union=Image.new("RGB", (PW + 1, PH))), "`control_image_union`"),
    (dict(image=torch.zeros(1, 24, 64)), "belong to FluxControlNetRepaintPipeline"),
    (dict(mask_image=torch.zeros(1, 24, 64)), "belong to FluxControlNetRepaintPipeline"),
    (dict(image=[Image.new("RGB", (PW, PH))] * 2), "one photo per call"),
    (dict(image=np.zeros([2, PH, PW, 3], dtype=np.uint8)), "one photo per call"),
    (dict(image=np.zeros([PH, PW, 3], dtype=np.float32)), "`image`: a PIL image, or a uint8 array"),
    (dict(image=None), "`image`"), (dict(output_type="jpeg"), "unsupported output_type"),
    (dict(strength=0.0), "number of pipeline steps"),
    (dict(height=96, width=64, image=np.zeros([100, PW, 3], dtype=np.uint8), mask_image=_box(10, 60, 10, 250, h=100), control_image=None,
          control_mask=None, control_position=None), "a working size that fits: width=96, height=32"),
    (dict(height=16, width=16, image=np.zeros([1000, 1000, 3], dtype=np.uint8), mask_image=_box(100, 900, 100, 900, h=1000, w=1000),
          control_image=None, control_mask=None, control_position=None), "more than a factor of 16"),
])
def test_refusals_before_any_device_work(no_native_call, bad, match):
    pipe = _pipe()
    with pytest.raises(ValueError, match=match):
        pipe(**_kw(**bad))
    assert_no_call_state(pipe)
    assert not {"_photo", "_photo_call", "_region", "_mask", "_padding_mask_crop", "_mask_blur"} & set(pipe.__dict__)


def test_a_call_without_a_prompt_is_refused_by_check_inputs(no_native_call):
    pipe = _pipe()
    with pytest.raises(ValueError, match="prompt"):
        pipe(**_kw(prompt_embeds=None, pooled_prompt_embeds=None))
    assert_no_call_state(pipe)


def test_the_accepted_inputs_reach_the_upload_with_the_region(no_native_call):
    """What ``_check_photo_inputs`` returns for PIL, array and tensor inputs: uint8 arrays at the photo's size, the mask (here the union
    of the lines' masks), the region; token tensors are left as they are."""
    pipe = _pipe()
    kw = _kw()
    lines = [_box(80, 100, 100, 160), _box(100, 120, 120, 150)]
    token_mask = torch.zeros(1, 24, 1)
    photo, mask, region, cond = pipe._check_photo_inputs(Image.fromarray(kw["image"]), None, [kw["control_image"][0], torch.zeros(1, 24, 128)], lines,
                                                         [np.asarray(lines[0]), torch.from_numpy(np.array(lines[1]))], None, None, 16, 4.0, "pil", H, W)
    assert np.array_equal(photo, kw["image"]) and photo.dtype == np.uint8
    assert np.array_equal(mask, np.maximum(np.asarray(lines[0]), np.asarray(lines[1]))) and region == (76, 64, 184, 136)
    assert cond["control_image"][0].shape == (PH, PW, 3) and cond["control_image"][1].shape == (1, 24, 128)
    assert all(a.shape == (PH, PW) and a.dtype == np.uint8 for a in cond["control_mask"] + cond["control_position"])
    assert cond["control_glyph"] is None and cond["control_image_union"] is None
    got = pipe._check_photo_inputs(kw["image"], _box(), None, [token_mask], None, None, None, 16, 4.0, "pil", H, W)
    assert got[3]["control_mask"][0] is token_mask and got[2] == (76, 64, 184, 136)


def test_signature_is_the_repaint_signature_plus_two():
    from reptext_amd.pipeline import CallExtensions, FluxControlNetPipeline
    from reptext_amd.pipeline_photo import FluxControlNetPhotoPipeline
    from reptext_amd.pipeline_repaint import FluxControlNetRepaintPipeline

    params = inspect.signature(FluxControlNetPhotoPipeline.__call__).parameters
    repaint = inspect.signature(FluxControlNetRepaintPipeline.__call__).parameters
    assert list(repaint) == BASE_PARAMS + ["image", "mask_image", "strength"]
    assert list(inspect.signature(FluxControlNetPipeline.__call__).parameters) == BASE_PARAMS
    assert list(params) == list(repaint) + ["padding_mask_crop", "mask_blur"]
    assert all(params[k].default == repaint[k].default for k in list(repaint)[1:])
    assert (params["padding_mask_crop"].default, params["mask_blur"].default) == (32, 4.0)
    assert (params["padding_mask_crop"].annotation, params["mask_blur"].annotation) in ((int, float), ("int", "float"))
    fields = [f.name for f in dataclasses.fields(CallExtensions)]
    assert len(fields) == 13 and not set(fields) & set(params) and not {"padding_mask_crop", "mask_blur"} & set(fields)
    assert issubclass(FluxControlNetPhotoPipeline, FluxControlNetRepaintPipeline)
    # the extensions are taken, any other keyword is a TypeError; the repaint pipeline does not take the two names
    with pytest.raises(TypeError, match="no_such_argument"):
        _pipe()(**_kw(), no_such_argument=1)
    from test_repaint_host import _kw as repaint_kw, _pipe as repaint_pipe
    for name in ("padding_mask_crop", "mask_blur"):
        with pytest.raises(TypeError, match=name):
            repaint_pipe()(**repaint_kw(), **{name: 1})


def test_the_shim_imports():
    import pipeline_flux_controlnet_photo as shim
    from reptext_amd import pipeline_photo

    assert shim.FluxControlNetPhotoPipeline is pipeline_photo.FluxControlNetPhotoPipeline
    assert shim.photo_crop_region is pipeline_photo.photo_crop_region and shim.min_padding_for_blur(4.0) == 12
    assert sorted(shim.__all__) == shim.__all__ and "FluxControlNetPhotoPipeline" in shim.__all__
    assert all(hasattr(shim, name) for name in shim.__all__)


def test_the_restatements_agree_with_themselves_where_they_are_exact():
    g = torch.Generator().manual_seed(0)
    photo = torch.randint(0, 256, (31, 45, 3), generator=g, dtype=torch.uint8)
    # a window resampled to its own size is the window
    r = resize_aa_ref(photo, (3, 2, 41, 29), (29, 41), 2.0, -1.0)
    assert torch.equal(r, 2.0 * (photo[2:31, 3:44].permute(2, 0, 1).double() / 255.0) - 1.0)
    assert aa_tap_count(41, 41) == 2 and aa_tap_count(200, 16) == 25 and aa_tap_count(1, 4) == 1 and aa_tap_count(9, 8) == 2
    # upscaling is plain bilinear
    up = resize_aa_ref(photo, (0, 0, 45, 31), (70, 90))
    plain = torch.nn.functional.interpolate(photo.permute(2, 0, 1)[None].double() / 255.0, size=(70, 90), mode="bilinear", align_corners=False)[0]
    assert float((up - plain).abs().max()) < 1e-12
    # alpha 0 is the photo, alpha 1 the generated image; outside the window the photo
    gen = torch.rand(3, 10, 20, generator=g).numpy() * 2.4 - 1.2
    window = (5, 7, 20, 10)
    zero = composite_ref(photo.numpy(), gen, np.zeros([10, 20]), window)
    one = composite_ref(photo.numpy(), gen, np.ones([10, 20]), window)
    assert np.array_equal(zero, photo.numpy().astype(np.float64))
    assert np.array_equal(one[7:17, 5:25], (np.clip(gen.astype(np.float64) / 2 + 0.5, 0, 1) * 255).transpose(1, 2, 0))
    inside = np.zeros([31, 45], dtype=bool); inside[7:17, 5:25] = True
    assert np.array_equal(one[~inside], photo.numpy()[~inside])
    # the blur: ones stay ones, zeros farther than R from the support, the weights' symmetry
    assert float(np.abs(gaussian_blur_ref(np.ones([20, 30]), 2.0) - 1.0).max()) < 1e-15
    box = np.zeros([37, 45]); box[15:22, 18:27] = 1.0
    blurred = gaussian_blur_ref(box, 2.0)
    assert float(blurred[:9].max()) == 0.0 and float(blurred[:, :12].max()) == 0.0 and float(blurred[9, 18]) > 0.0
    assert np.allclose(blurred, blurred[::-1, ::-1]) and abs(float(blurred.sum()) - 63.0) < 1e-9
