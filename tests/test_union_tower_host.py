"""Host side of the second ControlNet (pipe.controlnet_union, Union-Pro-2.0 beside the RepText tower): the active-step rule, the call
signature and every refusal, on CPU-constructed tiny models. No kernel runs here: the refusals come before any device work."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from test_true_cfg_host import assert_no_call_state

SMALL_T = dict(patch_size=1, in_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=1,
               joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
SMALL_CN = dict(SMALL_T, num_single_layers=0, extra_condition_channels=64)
SMALL_UN = dict(SMALL_T, num_single_layers=0)


def make_pipe(cls=None, union=SMALL_UN, controlnet=True, **extra):
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from reptext_amd.transformer import FluxTransformer2DModel

    tr = FluxTransformer2DModel(**SMALL_T, device="cpu", dtype=torch.bfloat16)
    cn = FluxControlNetModel(**SMALL_CN, device="cpu", dtype=torch.bfloat16) if controlnet else None
    pipe = (cls or FluxControlNetPipeline)(FlowMatchEulerDiscreteScheduler(), None, None, None, None, None, tr, cn, **extra)
    if union is not None:
        pipe.controlnet_union = FluxControlNetModel(**union, device="cpu", dtype=torch.bfloat16)
    return pipe


def call_kwargs(**over):
    kw = dict(prompt_embeds=torch.zeros(1, 8, 64, dtype=torch.bfloat16), pooled_prompt_embeds=torch.zeros(1, 32, dtype=torch.bfloat16),
              height=64, width=64, num_inference_steps=2, output_type="latent", control_image_union=torch.zeros(1, 16, 64, dtype=torch.bfloat16))
    kw.update(over)
    return kw


def test_active_step_rule_known_answers():
    from reptext_amd.pipeline import union_active_steps

    assert union_active_steps(28, 0.0, 0.8) == tuple(range(0, 22))
    assert union_active_steps(28, 0, 1) == tuple(range(28))
    assert union_active_steps(30, 0.15, 0.65) == tuple(range(5, 19))
    assert union_active_steps(3, 0.9, 0.1) == ()


def test_tower_schedule_known_answers():
    """``tower_schedule`` per step, as literal lists of (tower, table position). Towers are numbered union (if any), text lines, extra
    towers; U / T / X below name them for each case."""
    from reptext_amd.pipeline import tower_schedule, union_active_steps

    U, T = 0, 1
    assert tower_schedule(4, 30, 1, (1, 2)) == [[(T, 0)], [(U, 0), (T, 1)], [(U, 1), (T, 2)], [(T, 3)]]
    assert tower_schedule(3, 1, 1, (0, 1, 2)) == [[(U, 0), (T, 0)], [(U, 1)], [(U, 2)]]
    assert tower_schedule(3, 30, 0, (1,)) == [[], [(U, 0)], []]
    assert tower_schedule(3, 0, 1, (0,)) == [[(U, 0)], [], []]
    T0, T1, X = 0, 1, 2
    assert tower_schedule(3, 2, 2) == [[(T0, 0), (T1, 0)], [(T0, 1), (T1, 1)], []]
    assert tower_schedule(3, 2, 2, None, 0) == tower_schedule(3, 2, 2, (), 0) == tower_schedule(3, 2, 2)
    assert tower_schedule(3, 2, 2, None, 1) == [[(T0, 0), (T1, 0), (X, 0)], [(T0, 1), (T1, 1), (X, 1)], []]
    # an extra tower without a text line, or with the text towers switched off: nothing at any step
    assert tower_schedule(3, 2, 0, None, 1) == [[], [], []]
    assert tower_schedule(3, 0, 2, None, 1) == [[], [], []]
    # an empty guidance interval (start > end), fed through: no union tower anywhere, the text lines keep their numbers
    assert union_active_steps(3, 0.9, 0.1) == ()
    assert tower_schedule(3, 2, 2, union_active_steps(3, 0.9, 0.1)) == [[(T0, 0), (T1, 0)], [(T0, 1), (T1, 1)], []]


def test_call_signature_and_keywords():
    """The base ``__call__`` still reports the reference's parameter list; the four union keywords are taken by the base pipeline
    (they reach the refusal that names them) and are unknown to the inpaint pipeline."""
    from reptext_amd.pipeline import FluxControlNetPipeline
    from reptext_amd.pipeline_inpaint import FluxControlNetPipeline as Inpaint

    names = list(inspect.signature(FluxControlNetPipeline.__call__).parameters)
    assert names[0] == "self" and names[1:4] == ["prompt", "prompt_2", "height"] and names[-1] == "control_glyph"
    assert len(names) == 28 and not any("union" in n for n in names)
    pipe = make_pipe(union=None)
    assert pipe.controlnet_union is None and "controlnet_union" not in pipe.components
    with pytest.raises(ValueError, match="control_image_union"):       # accepted as keywords, refused for the missing tower
        pipe(**call_kwargs(controlnet_conditioning_scale_union=0.7, control_guidance_start_union=0.0, control_guidance_end_union=0.8))
    assert_no_call_state(pipe)
    inp = make_pipe(cls=Inpaint, controlnet_inpaint=None)
    base_kw = call_kwargs()
    del base_kw["control_image_union"]
    for k, v in dict(control_image_union=torch.zeros(1, 16, 64), controlnet_conditioning_scale_union=0.7, control_guidance_start_union=0.1,
                     control_guidance_end_union=0.8).items():
        with pytest.raises(TypeError, match=k):
            inp(**base_kw, **{k: v})


def test_components_to_and_lora_models_see_the_union_tower():
    pipe = make_pipe()
    assert pipe.components["controlnet_union"] is pipe.controlnet_union
    assert list(pipe.components)[:8] == ["scheduler", "vae", "text_encoder", "tokenizer", "text_encoder_2", "tokenizer_2", "transformer", "controlnet"]
    pipe.to(dtype=torch.float32)
    assert pipe.controlnet_union.x_embedder.weight.dtype == torch.float32
    pipe.controlnet_union._lora = object()                              # what a loaded adapter leaves on a model
    assert pipe.controlnet_union in pipe._lora_models()


def test_refusals_name_the_argument():
    from reptext_amd.controlnet import FluxControlNetModel

    # no second tower on the pipeline
    with pytest.raises(ValueError, match="control_image_union"):
        make_pipe(union=None)(**call_kwargs())
    # no first tower
    with pytest.raises(ValueError, match="control_image_union"):
        make_pipe(controlnet=False)(**call_kwargs())
    # deeper than the first tower: double blocks, single blocks
    with pytest.raises(ValueError, match="control_image_union.*more than the first tower"):
        make_pipe(union=dict(SMALL_UN, num_layers=2))(**call_kwargs())
    with pytest.raises(ValueError, match="control_image_union.*more than the first tower"):
        make_pipe(union=dict(SMALL_UN, num_single_layers=1))(**call_kwargs())
    # another inner_dim
    with pytest.raises(ValueError, match="control_image_union.*inner_dim"):
        make_pipe(union=dict(SMALL_UN, num_attention_heads=2))(**call_kwargs())
    # packed hint: width, batch, N (64x64 pixels are 4x4 = 16 rows)
    pipe = make_pipe()
    with pytest.raises(ValueError, match="control_image_union.*width"):
        pipe(**call_kwargs(control_image_union=torch.zeros(1, 16, 128, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="control_image_union.*batch"):
        pipe(**call_kwargs(control_image_union=torch.zeros(3, 16, 64, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="control_image_union.*N = 12"):
        pipe(**call_kwargs(control_image_union=torch.zeros(1, 12, 64, dtype=torch.bfloat16)))
    # an image without a VAE to encode it
    with pytest.raises(ValueError, match="control_image_union.*VAE"):
        pipe(**call_kwargs(control_image_union=torch.zeros(1, 3, 64, 64)))
    # Union v1 (mode embedding) stays out of scope
    pipe.controlnet_union = FluxControlNetModel(**dict(SMALL_UN, num_mode=10), device="cpu", dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        pipe(**call_kwargs())


def test_from_pretrained_takes_a_union_tower(tmp_path):
    """``controlnet_union=`` of from_pretrained: a model instance is taken as it is (a directory or cached hub id goes through
    FluxControlNetModel.from_pretrained like ``controlnet=``)."""
    from reptext_amd.controlnet import FluxControlNetModel
    from reptext_amd.pipeline import FluxControlNetPipeline

    src = make_pipe()
    un = FluxControlNetModel(**SMALL_UN, device="cpu", dtype=torch.bfloat16)
    pipe = FluxControlNetPipeline.from_pretrained(str(tmp_path), transformer=src.transformer, vae=SimpleNamespace(config=SimpleNamespace(block_out_channels=[1] * 4)), controlnet=src.controlnet,
                                                  controlnet_union=un)
    assert pipe.controlnet_union is un and pipe.components["controlnet_union"] is un
