"""CPU tests of the negative prompt (true CFG) in the text-to-image pipeline: every refusal by argument name and before any native
call, the rule that switches CFG on, the unchanged ``__call__`` signatures, the inpaint pipeline's refusal of ``true_cfg_scale``, and
the choice of the negative image prompt with a stub encoder. No kernel runs here."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ip_adapter_reference as ipr  # noqa: E402

CFG = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=1, attention_head_dim=128, num_attention_heads=1,
           joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
C, E = 64, 32
# PIPE:751-781 and INP:846-883: the parameter lists the reference's two __call__s have
BASE_PARAMS = ["self", "prompt", "prompt_2", "height", "width", "num_inference_steps", "timesteps", "guidance_scale", "control_guidance_start",
               "control_guidance_end", "control_image", "control_mode", "controlnet_conditioning_scale", "controlnet_conditioning_step",
               "num_images_per_prompt", "generator", "latents", "prompt_embeds", "pooled_prompt_embeds", "output_type", "return_dict",
               "joint_attention_kwargs", "callback_on_step_end", "callback_on_step_end_tensor_inputs", "max_sequence_length", "control_mask",
               "control_position", "control_glyph"]
INPAINT_PARAMS = BASE_PARAMS[:3] + ["true_guidance_scale", "negative_prompt", "negative_prompt_2"] + BASE_PARAMS[3:] + \
    ["control_image_inpaint", "control_mask_inpaint", "controlnet_conditioning_scale_inpaint", "negative_prompt_embeds",
     "negative_pooled_prompt_embeds"]


@pytest.fixture
def no_native_call(monkeypatch):
    from reptext_amd import native

    def refuse(name, *args):
        raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(native, "call", refuse)


def _pipe(inpaint=False):
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as InpaintPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**CFG, device="cpu", dtype=torch.bfloat16)
    if inpaint:
        return InpaintPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, None, None)
    return FluxControlNetPipeline(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, None)


def assert_no_call_state(pipe):
    """Nothing of a call is left on the pipeline: the one attribute that carries a call's extension arguments is None again, and none of
    the six attributes that once carried them and what was derived from them exists."""
    assert pipe._call_extensions is None
    assert not {"_ip_call_args", "_ip_embeds", "_union_call_args", "_union", "_cfg_call_args", "_cfg_scale"} & set(pipe.__dict__)


def _kw(B=1, T=8):
    return dict(prompt_embeds=torch.zeros(B, T, C), pooled_prompt_embeds=torch.zeros(B, 32), height=64, width=64, num_inference_steps=1)


def test_signatures_are_the_references():
    from reptext_amd import pipeline
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as InpaintPipeline

    assert list(inspect.signature(FluxControlNetPipeline.__call__).parameters) == BASE_PARAMS
    assert list(inspect.signature(InpaintPipeline.__call__).parameters) == INPAINT_PARAMS
    assert pipeline.TRUE_CFG_ARGUMENTS == ("negative_prompt", "negative_prompt_2", "true_cfg_scale", "negative_prompt_embeds",
                                           "negative_pooled_prompt_embeds", "negative_ip_adapter_image", "negative_ip_adapter_image_embeds")
    assert not set(pipeline.TRUE_CFG_ARGUMENTS) & set(BASE_PARAMS)


def test_the_rule_that_switches_cfg_on():
    from reptext_amd.pipeline import do_true_cfg

    e = torch.zeros(1, 8, C)
    assert do_true_cfg(3.5, "blurry") and do_true_cfg(1.01, ["a", "b"]) and do_true_cfg(2.0, None, e, e)
    assert do_true_cfg(2.0, "") is True                               # an empty negative prompt is a negative prompt
    assert not do_true_cfg(1.0, "blurry") and not do_true_cfg(0.5, "blurry") and not do_true_cfg(1.0, None, e, e)
    assert not do_true_cfg(3.5) and not do_true_cfg(3.5, None, e, None) and not do_true_cfg(3.5, None, None, e)


@pytest.mark.parametrize("bad, name", [
    (dict(negative_prompt_embeds=torch.zeros(1, 8, C)), "negative_pooled_prompt_embeds"),                       # only one of the two
    (dict(negative_pooled_prompt_embeds=torch.zeros(1, 32)), "negative_prompt_embeds"),
    (dict(negative_prompt="blurry", negative_prompt_embeds=torch.zeros(1, 8, C), negative_pooled_prompt_embeds=torch.zeros(1, 32)),
     "negative_prompt"),                                                                                          # text and embeds
    (dict(negative_prompt_2="blurry", negative_prompt_embeds=torch.zeros(1, 8, C), negative_pooled_prompt_embeds=torch.zeros(1, 32)),
     "negative_prompt_2"),
    (dict(negative_prompt=["a", "b"]), "negative_prompt"),                                                       # 2 negatives, batch 1
    (dict(negative_prompt="a", negative_prompt_2=["a", "b", "c"]), "negative_prompt_2"),
    (dict(negative_prompt=7), "negative_prompt"),
    (dict(negative_prompt_embeds=torch.zeros(1, 9, C), negative_pooled_prompt_embeds=torch.zeros(1, 32)), "negative_prompt_embeds"),
    (dict(negative_prompt_embeds=torch.zeros(2, 8, C), negative_pooled_prompt_embeds=torch.zeros(1, 32)), "negative_prompt_embeds"),
    (dict(negative_prompt_embeds=torch.zeros(1, 8, C), negative_pooled_prompt_embeds=torch.zeros(1, 48)), "negative_pooled_prompt_embeds"),
    (dict(negative_ip_adapter_image=object()), "negative_ip_adapter_image"),                                     # no positive image prompt
    (dict(negative_ip_adapter_image_embeds=torch.zeros(1, 1, E)), "negative_ip_adapter_image_embeds"),
], ids=lambda v: v if isinstance(v, str) else "+".join(v))
@pytest.mark.parametrize("scale", [1.0, 3.5])
def test_refusals_name_the_argument_before_any_device_work(no_native_call, bad, name, scale):
    """Refused whether or not the scale switches CFG on, with the argument's name in backticks, before any entry point is reached."""
    with pytest.raises(ValueError, match=f"`{name}`"):
        _pipe()(**_kw(), true_cfg_scale=scale, **bad)


def test_positive_and_negative_image_prompts_are_checked_together(no_native_call):
    pipe = _pipe()
    pipe.load_ip_adapter(ipr.init_ip_params(CFG, n_tokens=4, embed_dim=E, seed=6))
    pos = torch.zeros(1, 1, E)
    with pytest.raises(ValueError, match="either negative_ip_adapter_image or negative_ip_adapter_image_embeds"):
        pipe(**_kw(), ip_adapter_image_embeds=pos, negative_ip_adapter_image=object(), negative_ip_adapter_image_embeds=pos)
    # the positive one inside joint_attention_kwargs counts as a positive one: the next refusal in line is the width check of the embeds
    with pytest.raises(ValueError, match="width 48"):
        pipe(**_kw(), joint_attention_kwargs={"ip_adapter_image_embeds": torch.zeros(1, 1, 48)}, negative_ip_adapter_image_embeds=pos)
    assert_no_call_state(pipe)


def test_inpaint_pipeline_does_not_take_true_cfg_scale():
    with pytest.raises(TypeError, match="true_cfg_scale"):
        _pipe(inpaint=True)(**_kw(), true_cfg_scale=2.0)
    with pytest.raises(TypeError, match="negative_ip_adapter_image"):
        _pipe(inpaint=True)(**_kw(), negative_ip_adapter_image=object())


def test_a_scale_without_a_negative_prompt_logs_one_line_and_stays_off(capsys):
    from reptext_amd.pipeline import CallExtensions

    pipe = _pipe()
    ext = CallExtensions(negative_prompt=None, negative_prompt_2=None, true_cfg_scale=3.5, negative_prompt_embeds=None,
                         negative_pooled_prompt_embeds=None, negative_ip_adapter_image=None, negative_ip_adapter_image_embeds=None)
    kw = _kw()
    assert pipe._check_true_cfg_inputs(ext, kw["prompt_embeds"], kw["pooled_prompt_embeds"], 1, None) is False
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "true_cfg_scale" in err and "negative prompt" in err
    ext.true_cfg_scale = 1.0
    ext.negative_prompt = "blurry"
    assert pipe._check_true_cfg_inputs(ext, kw["prompt_embeds"], kw["pooled_prompt_embeds"], 1, None) is False
    ext.true_cfg_scale = 1.5
    assert pipe._check_true_cfg_inputs(ext, kw["prompt_embeds"], kw["pooled_prompt_embeds"], 1, None) is True
    assert capsys.readouterr().err == ""
    # no extension passed at all, which is what a direct _denoise user amounts to
    assert pipe._check_true_cfg_inputs(CallExtensions(), kw["prompt_embeds"], kw["pooled_prompt_embeds"], 1, None) is False
    assert capsys.readouterr().err == ""


def test_negative_prompt_is_encoded_by_the_same_path(monkeypatch):
    """negative_prompt_2 defaults to negative_prompt, one string serves the batch, num_images_per_prompt and max_sequence_length are
    passed on; the result must have the positive embeddings' shape."""
    from reptext_amd.pipeline import CallExtensions

    pipe = _pipe()
    seen = []

    def encode_prompt(prompt, prompt_2, device=None, num_images_per_prompt=1, max_sequence_length=512, **kw):
        seen.append((prompt, prompt_2, num_images_per_prompt, max_sequence_length))
        n = len(prompt) * num_images_per_prompt
        return torch.ones(n, max_sequence_length, C), torch.ones(n, 32), None

    monkeypatch.setattr(pipe, "encode_prompt", encode_prompt)
    args = dict(negative_prompt="blurry", negative_prompt_2=None, true_cfg_scale=2.0, negative_prompt_embeds=None,
                negative_pooled_prompt_embeds=None, negative_ip_adapter_image=None, negative_ip_adapter_image_embeds=None)
    ext = CallExtensions(**args)
    pe, pooled = torch.zeros(4, 8, C, dtype=torch.bfloat16), torch.zeros(4, 32, dtype=torch.bfloat16)
    npe, npooled = pipe._encode_negative_prompt(ext, pe, pooled, 2, 2, 8, "cpu")
    assert seen == [(["blurry", "blurry"], ["blurry", "blurry"], 2, 8)]
    assert npe.shape == pe.shape and npooled.shape == pooled.shape and npe.dtype == torch.bfloat16 and float(npe.float().min()) == 1.0
    ext = CallExtensions(**dict(args, negative_prompt=["a", "b"], negative_prompt_2="c"))
    pipe._encode_negative_prompt(ext, pe, pooled, 2, 2, 8, "cpu")
    assert seen[-1] == (["a", "b"], ["c", "c"], 2, 8)
    with pytest.raises(ValueError, match="`negative_prompt_embeds`"):           # T = 8 positive embeddings against max_sequence_length 16
        pipe._encode_negative_prompt(ext, pe, pooled, 2, 2, 16, "cpu")
    # embeddings as passed are taken as they are
    ext = CallExtensions(**dict(args, negative_prompt=None, negative_prompt_embeds=pe + 2, negative_pooled_prompt_embeds=pooled + 3))
    n = len(seen)
    npe, npooled = pipe._encode_negative_prompt(ext, pe, pooled, 2, 2, 8, "cpu")
    assert len(seen) == n and float(npe.float().min()) == 2.0 and float(npooled.float().min()) == 3.0


def test_the_negative_image_prompt_rule_with_a_stub_encoder(monkeypatch):
    """negative embeds if given; else the negative image through encode_image; else an all-black image through the same encoder when
    the positive prompt was an image; else a zero embedding."""
    from PIL import Image

    from reptext_amd.pipeline import CallExtensions

    pipe = _pipe()
    pipe.image_encoder = type("Enc", (), {"config": type("Cfg", (), {"image_size": 24})()})()
    seen = []

    def encode_image(image, device=None, num_images_per_prompt=1):
        seen.append(image)
        return torch.full((1, E), 5.0)

    monkeypatch.setattr(pipe, "encode_image", encode_image)
    none = dict(negative_ip_adapter_image=None, negative_ip_adapter_image_embeds=None)
    negative = lambda ext: pipe._negative_ip_embeds(ext, positive, 2, "cpu")
    positive = torch.ones(2, E, dtype=torch.bfloat16)
    picture = Image.new("RGB", (8, 8), (200, 10, 10))
    # 1. explicit embeds win, also over a positive image; one row serves the batch
    out = negative(CallExtensions(ip_adapter_image=picture, **dict(none, negative_ip_adapter_image_embeds=torch.full((1, 1, E), 7.0))))
    assert seen == [] and out.shape == (2, E) and out.dtype == torch.bfloat16 and float(out.float().min()) == 7.0
    # 2. a negative image goes through the encoder
    out = negative(CallExtensions(ip_adapter_image=picture, **dict(none, negative_ip_adapter_image=picture)))
    assert seen == [picture] and out.shape == (2, E) and float(out.float().min()) == 5.0
    # 3. nothing negative, the positive was an image: an all-black image at the encoder's size through the same encoder
    out = negative(CallExtensions(ip_adapter_image=picture, **none))
    assert len(seen) == 2 and isinstance(seen[1], Image.Image) and seen[1].size == (24, 24) and seen[1].getextrema() == ((0, 0),) * 3
    assert float(out.float().min()) == 5.0
    # 4. nothing negative, the positive were embeds: zeros, no encoder run
    out = negative(CallExtensions(ip_adapter_image_embeds=positive, **none))
    assert len(seen) == 2 and out.shape == (2, E) and float(out.float().abs().max()) == 0.0
    # refusals
    with pytest.raises(ValueError, match="negative_ip_adapter_image_embeds: width 48"):
        negative(CallExtensions(ip_adapter_image_embeds=positive, **dict(none, negative_ip_adapter_image_embeds=torch.zeros(1, 1, 48))))
    with pytest.raises(ValueError, match="negative_ip_adapter_image_embeds: batch 3"):
        negative(CallExtensions(ip_adapter_image_embeds=positive, **dict(none, negative_ip_adapter_image_embeds=torch.zeros(3, 1, E))))
    pipe.image_encoder = None
    with pytest.raises(NotImplementedError, match="negative_ip_adapter_image_embeds"):
        negative(CallExtensions(ip_adapter_image_embeds=positive, **dict(none, negative_ip_adapter_image=picture)))


def test_token_masks_per_image_are_taken_as_they_are():
    """control_mask entries that are [B,N,1] tensors are token masks, one per image (an extension like packed hints); PIL masks still
    give the shared [1,N,1] form."""
    from PIL import Image

    pipe = _pipe()
    m = torch.rand(2, 16, 1)
    out = pipe._region_masks([m, Image.new("L", (64, 64), 255)], "cpu", torch.float32)
    assert torch.equal(out[0], m) and out[1].shape == (1, 16, 1) and float(out[1].min()) == 1.0
